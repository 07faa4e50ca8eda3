// In-launch hand-offs of the persistent kernels: 8-byte {tag:32 | fp32} granules published with
// relaxed atomic stores and polled with L1-bypassing loads (MI355X_MICROARCH.md "Valid forms": the
// fence-free hand-off), every wait bounded on wall_clock64, and the set-up exchange of XCC ids from
// which a workgroup takes its rank.  The only home of that protocol; its users are
// resident_decoder.hip (Tacotron2, batch 1), resident_batch.hip (batches of 2-8),
// tacotron_resident.hip (Tacotron / GST), encoder_resident.hip (both encoder kernels) and the
// persistent Griffin-Lim loop of griffin_lim.hip.  DESIGN.md "Hand-off primitives" lists every
// wait's policy.
#pragma once
#include <hip/hip_runtime.h>

namespace tts {
namespace handoff {

typedef unsigned long long u64;
typedef __attribute__((address_space(1))) u64 gu64;
typedef __attribute__((address_space(1))) int gint;
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
constexpr int SC1_VOLATILE = (int)0x80000010u;  // buffer aux: sc1 (bit 4) | volatile (bit 31)
constexpr int VOLATILE_AUX = (int)0x80000000u;  // buffer aux: volatile only (default cache policy)
constexpr int OOB_OFF = 0x7FFFFFF0;             // past every buffer: reads 0, no access

#ifndef RES_SLEEP
#define RES_SLEEP 0  // s_sleep between polls: 0 measured 11.03 -> 10.70 us per step (tools/dec_ab.sh)
#endif

// the XCD (0..7) this wave runs on
__device__ __forceinline__ int xcc_id() {
    int xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    return xcc & 7;
}

// ---- stores and loads; the scope of a store is in its name
// Device-wide edge: written through to memory.
__device__ __forceinline__ void publish_agent(u64* g, unsigned tag, float v) {
    __hip_atomic_store((gu64*)g, ((u64)tag << 32) | (u64)__float_as_uint(v), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}
// Same-XCD edge: a workgroup-scope store (global_store ... sc0) keeps the line in the XCD's L2,
// which every CU of that XCD reads with the agent-scope (sc1, L1-bypassing) loads of the sweeps.
// A reader on another XCD never sees it.
__device__ __forceinline__ void publish_xcd(u64* g, unsigned tag, float v) {
    __hip_atomic_store((gu64*)g, ((u64)tag << 32) | (u64)__float_as_uint(v), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ u64 peek(u64* g) {
    return __hip_atomic_load((gu64*)g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned peek32(const unsigned* g) {
    return __hip_atomic_load((__attribute__((address_space(1))) unsigned*)g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void publish32_agent(unsigned* g, unsigned v) {
    __hip_atomic_store((__attribute__((address_space(1))) unsigned*)g, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- a launch's status word
// The first failure of a launch wins (the other workgroups then time out in cascade); its step
// and workgroup go to status[1], status[2] (diagnostics).
__device__ __forceinline__ void fail(int* status, int code, int step = -1) {
    int expected = 0;
    if (__hip_atomic_compare_exchange_strong((gint*)status, &expected, code, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT)) {
        __hip_atomic_store((gint*)status + 1, step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store((gint*)status + 2, (int)blockIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
// The last writer wins: a plain store of a word the caller builds (a raw code, or salt << 8 | code
// where the host does not clear the word between launches).
__device__ __forceinline__ void fail_word(int* status, int word) {
    __hip_atomic_store((gint*)status, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- the bounded poll: every wait of the Tacotron / GST decoder, the two encoder kernels and the
// Griffin-Lim loop is a lambda on this loop
// One wave calls poll() (-> this lane's tags are in) until it holds on every lane: true.  false
// once `tmo` wall-clock ticks have passed (the caller flags the error, the grid drains); what
// poll() wrote on its last call stands either way.  SLEEP: s_sleep between polls (0: none).
//   AHEAD false: the clock is first read after the first failed poll and compared on the spins
//     with (spin & 31) == CHECK_AT, spin 0 excepted.  AHEAD true: the deadline is taken before the
//     first poll and compared on those spins, spin 0 included.  EACH: ahead, and compared after
//     every failed poll, so the bound holds to a poll's length however short `tmo` is.
template <int CHECK_AT, int SLEEP, bool EACH = false, bool AHEAD = EACH, typename Poll>
__device__ __forceinline__ bool poll_until(Poll poll, long long tmo) {
    static_assert(AHEAD || !EACH, "EACH reads the clock ahead");
    long long t_end = AHEAD ? (long long)wall_clock64() + tmo : 0;
    for (int spin = 0;; ++spin) {
        if (__all(poll())) return true;
        if (!AHEAD && spin == 0) {
            t_end = (long long)wall_clock64() + tmo;
        } else if ((EACH || (spin & 31) == CHECK_AT) && (long long)wall_clock64() > t_end) {
            return false;
        }
        if (SLEEP) __builtin_amdgcn_s_sleep(SLEEP);
    }
}
// n x s_sleep(T) ahead of a wait's first poll: a poll storm from every CU the moment it has
// published slows the stores it waits for
template <int T>
__device__ __forceinline__ void first_poll_delay(int n) {
    for (int i = 0; i < n; ++i) __builtin_amdgcn_s_sleep(T);
}

// One wave polls its N granules per lane (idx(i) < 0: none) until every tag equals `tag`; v[i] =
// the values.  No branch in a poll: every load is issued (a slot with idx < 0 re-reads slot 0 and
// is ignored), so the N loads are in flight together, and `ok` is formed without short-circuit
// branches.  CHECK_AT and SLEEP as poll_until (the caller names its policy); `first_sleep` x
// s_sleep(FIRST_T) ahead of the first poll.
template <int N, int CHECK_AT, int SLEEP, int FIRST_T, typename F>
__device__ __forceinline__ bool sweep_flat(u64* g, unsigned tag, float (&v)[N], F idx, long long tmo, int first_sleep = 0) {
    first_poll_delay<FIRST_T>(first_sleep);
    return poll_until<CHECK_AT, SLEEP>(
        [&] {
            bool ok = true;
            u64 x[N];
#pragma unroll
            for (int i = 0; i < N; ++i) {
                const int k = idx(i);
                x[i] = peek(g + (k >= 0 ? k : 0));
            }
#pragma unroll
            for (int i = 0; i < N; ++i) {
                v[i] = __uint_as_float((unsigned)x[i]);
                ok = ok & ((idx(i) < 0) | ((unsigned)(x[i] >> 32) == tag));
            }
            return ok;
        },
        tmo);
}

// ---- the two Tacotron2 decoders' waits (resident_decoder.hip, resident_batch.hip), written out
// These kernels run with a full register file and their weights are live across every wait: on
// poll_until and xcd_census their step loops were allocated differently and measured 0.5-1.7 %
// slower (profiles/handoff_refactor_ab.txt), so they keep the loops below and their own set-up.
// One wave polls its N granules per lane (idx(i) < 0: none) until every tag equals tag(i);
// false after `tmo` wall-clock ticks (the caller flags the error, the grid drains).  The clock is
// read after the first failed poll and then every 32nd; EACH (a wait off every hot path, such as a
// launch's set-up exchange): read ahead of the first poll and after every failed one, so the
// bound holds to a poll's length however short `tmo` is.
template <int N, bool EACH = false, typename F, typename T>
__device__ __forceinline__ bool sweep2(u64* g, F idx, T tag, float (&v)[N], long long tmo) {
    long long t_end = EACH ? (long long)wall_clock64() + tmo : 0;
    for (int spin = 0;; ++spin) {
        bool ok = true;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int k = idx(i);
            if (k >= 0) {
                const u64 x = peek(g + k);
                v[i] = __uint_as_float((unsigned)x);
                ok = ok && (unsigned)(x >> 32) == tag(i);
            }
        }
        if (__all(ok)) return true;
        if (!EACH && spin == 0) {
            t_end = (long long)wall_clock64() + tmo;
        } else if ((EACH || (spin & 31) == 0) && (long long)wall_clock64() > t_end) {
            return false;
        }
        if (RES_SLEEP) __builtin_amdgcn_s_sleep(RES_SLEEP);
    }
}
// One wave polls its N granules per lane (idx(i) < 0: none) until every tag equals `tag`;
// false after `tmo` wall-clock ticks (the caller flags the error, the grid drains).
template <int N, bool EACH = false, typename F>
__device__ __forceinline__ bool sweep(u64* g, unsigned tag, float (&v)[N], F idx, long long tmo) {
    return sweep2<N, EACH>(g, idx, [&](int) { return tag; }, v, tmo);
}

// Granule pairs: every gather of the step loop reads ONE 16-byte pair (2 granules) per lane, an
// sc1 buffer load (L1-bypassing; volatile, so every poll re-issues it).  A poll's latency grows
// with the loads per lane (tools/microbench/edge.hip, round 4: device-wide 1024 granules 2.31 us per
// edge with 4 x 8-byte loads per lane on 4 waves, 1.60-1.63 with one pair or two granules per lane
// on 8 waves; XCD-local 256 granules 1.14 us with 4 per lane on one wave, 0.47 with one pair per
// lane on 2 waves).  Each 8-byte half is written whole by one store, so a pair is never torn
// within a half (MI355X_MICROARCH.md "Valid forms", R2's granule); both tags are checked.
// One wave polls one pair per lane at granule slot `slot` (even; < 0: none) until its tags equal
// `tag` (the second half only when `both`); v0/v1 = the two values.  false after `tmo` ticks.
__device__ __forceinline__ bool sweep_pair(__amdgpu_buffer_rsrc_t r, int slot, bool both, unsigned tag, float& v0,
                                           float& v1, long long tmo) {
    long long t_end = 0;
    for (int spin = 0;; ++spin) {
        bool ok = true;
        if (slot >= 0) {
            const u32x4 x = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(r, slot * 8, 0, SC1_VOLATILE));
            v0 = __uint_as_float(x.x);
            v1 = __uint_as_float(x.z);
            ok = x.y == tag && (!both || x.w == tag);
        }
        if (__all(ok)) return true;
        if (spin == 0) {
            t_end = (long long)wall_clock64() + tmo;
        } else if ((spin & 31) == 0 && (long long)wall_clock64() > t_end) {
            return false;
        }
        if (RES_SLEEP) __builtin_amdgcn_s_sleep(RES_SLEEP);
    }
}

// One wave polls one granule per lane at granule slot `slot` (< 0: none) until its tag equals
// `tag`: the same sc1 buffer load, 8 bytes.  false once `tmo` ticks have passed since the call.
// The clock is read ahead of the first poll (one scalar load, in flight beside it, consumed only
// if that poll fails): this gather follows useful work and never spins 32 times, so a timeout
// counted from the first failed poll and checked every 32nd would not bound it.
__device__ __forceinline__ bool sweep_one(__amdgpu_buffer_rsrc_t r, int slot, unsigned tag, float& v, long long tmo) {
    const long long t_end = (long long)wall_clock64() + tmo;
    for (int spin = 0;; ++spin) {
        bool ok = true;
        if (slot >= 0) {
            const u32x2 x = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(r, slot * 8, 0, SC1_VOLATILE));
            v = __uint_as_float(x.x);
            ok = x.y == tag;
        }
        if (__all(ok)) return true;
        if ((spin & 31) == 0 && (long long)wall_clock64() > t_end) return false;
        if (RES_SLEEP) __builtin_amdgcn_s_sleep(RES_SLEEP);
    }
}
// sweep_one with a second granule on the lanes whose `slot2` >= 0 (tag `tag2`, value v2): a word
// published long before the awaited granules, taken in the same bounded sweep.  Both loads of a
// poll are issued before either is consumed, the early word's first (vmcnt counts in order: its
// round trip lies inside the awaited granule's).  A lane without a second granule loads past the
// buffer (no access).  in2: this lane's second tag was in at the last poll (the caller's fail code).
__device__ __forceinline__ bool sweep_one_and(__amdgpu_buffer_rsrc_t r, int slot, unsigned tag, float& v, int slot2,
                                              unsigned tag2, float& v2, bool& in2, long long tmo) {
    const long long t_end = (long long)wall_clock64() + tmo;
    const int off2 = slot2 >= 0 ? slot2 * 8 : OOB_OFF;
    for (int spin = 0;; ++spin) {
        const u32x2 y = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(r, off2, 0, SC1_VOLATILE));
        const u32x2 x = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(r, slot * 8, 0, SC1_VOLATILE));
        v = __uint_as_float(x.x);
        v2 = __uint_as_float(y.x);
        in2 = (slot2 < 0) | (y.y == tag2);
        if (__all((x.y == tag) & in2)) return true;
        if ((spin & 31) == 0 && (long long)wall_clock64() > t_end) return false;
        if (RES_SLEEP) __builtin_amdgcn_s_sleep(RES_SLEEP);
    }
}

// Poll NP consecutive granule pairs from even slot `base` (thread i of the THREADS-wide workgroup: pairs i, i + THREADS, ...): every
// poll issues all of the thread's loads before one wait; the values go to dst[2p], dst[2p + 1]
// once every pair of the wave carries `tag`.  false after the timeout.
template <int NP, int THREADS>
__device__ __forceinline__ bool gather_pairs(__amdgpu_buffer_rsrc_t r, int base, unsigned tag, float* dst, long long tmo,
                                             int first_sleep = 0) {
    static_assert(NP % THREADS == 0, "whole pairs per thread");
    constexpr int MAXP = NP / THREADS;
    const int tid = threadIdx.x;
    long long t_end = 0;
    // (a poll storm from every CU the moment it has published slows the stores it waits for)
    for (int i = 0; i < first_sleep; ++i) __builtin_amdgcn_s_sleep(4);
    for (int spin = 0;; ++spin) {
        u32x4 x[MAXP];
#pragma unroll
        for (int i = 0; i < MAXP; ++i)
            x[i] = __builtin_bit_cast(
                u32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (base + 2 * (tid + i * THREADS)) * 8, 0, SC1_VOLATILE));
        bool ok = true;
#pragma unroll
        for (int i = 0; i < MAXP; ++i) ok = ok && x[i].y == tag && x[i].w == tag;
        if (__all(ok)) {
#pragma unroll
            for (int i = 0; i < MAXP; ++i)
                *reinterpret_cast<float2*>(dst + 2 * (tid + i * THREADS)) = float2{__uint_as_float(x[i].x), __uint_as_float(x[i].z)};
            return true;
        }
        if (spin == 0) {
            t_end = (long long)wall_clock64() + tmo;
        } else if ((spin & 31) == 0 && (long long)wall_clock64() > t_end) {
            return false;
        }
    }
}

// ---- XCD census: the set-up exchange of a 256-workgroup launch
// Workgroup c publishes its XCC id into table[c] (device-wide) and wave 0 sweeps the 256 entries,
// 4 per lane (all four loads issued, then the compares), under the caller's wait policy (CHECK_AT,
// SLEEP, EACH as poll_until).  The whole workgroup calls it; the result is valid on wave 0 only,
// and everything it gives but `raw` is wave-uniform: ok, the rank, and the eight per-XCD counts
// through count().  Which counts make a placement good is the caller's rule.
struct XcdCensus {
    bool ok;     // every entry arrived within tmo (else the rest is from a partial table)
    int rank;    // workgroups of this one's XCD with a lower index
    int raw[4];  // XCC ids of workgroups 4 lane .. 4 lane + 3
    // workgroups on XCD x (ballots: called by the whole wave); the eight counts are formed where
    // they are asked for, so a kernel whose registers are full at set-up holds none of them
    __device__ __forceinline__ int count(int x) const {
        int n = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) n += __popcll(__ballot(raw[i] == x));
        return n;
    }
    // XCC id of workgroup 0
    __device__ __forceinline__ int first_xcd() const { return __builtin_amdgcn_readfirstlane(raw[0]); }
};
template <int CHECK_AT, int SLEEP, bool EACH = false>
__device__ __forceinline__ XcdCensus xcd_census(u64* table, int c, int xcc, unsigned tag, long long tmo) {
    const int tid = threadIdx.x, lane = tid & 63;
    XcdCensus s = {};
    if (tid == 0) publish_agent(table + c, tag, __int_as_float(xcc));
    if (__builtin_amdgcn_readfirstlane(tid >> 6) == 0) {
        s.ok = poll_until<CHECK_AT, SLEEP, EACH>(
            [&] {
                u64 x[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) x[i] = peek(table + lane * 4 + i);
                bool ok = true;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    s.raw[i] = (int)x[i] & 7;
                    ok = ok & ((unsigned)(x[i] >> 32) == tag);
                }
                return ok;
            },
            tmo);
#pragma unroll
        for (int i = 0; i < 4; ++i) s.rank += __popcll(__ballot(s.raw[i] == xcc && lane * 4 + i < c));
    }
    return s;
}

}  // namespace handoff
}  // namespace tts
