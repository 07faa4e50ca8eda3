// Host-only helpers shared by the API files: checkpoint weight lookup, a handle's device
// allocations, the step graphs of the multi-launch decoders, environment knobs.
#pragma once
#include <cstdlib>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "sgemm.h"

// Returns the status of x from the enclosing function unless it is TTS_OK.
#define TTS_TRY(x)                            \
    do {                                      \
        if (tts_status st_ = (x)) return st_; \
    } while (0)

namespace tts {

// Checkpoint tensors by key.  get() checks the element count (numel < 0: any size) and leaves the
// reason in the error string when it returns null.
struct WeightMap {
    std::unordered_map<std::string, std::pair<const float*, int64_t>> m;
    WeightMap(const tts_tensor* tensors, int n) {
        for (int i = 0; i < n; ++i) m[tensors[i].key] = {tensors[i].data, tensors[i].numel};
    }
    const float* get(const std::string& k, int64_t numel) const {
        auto it = m.find(k);
        if (it == m.end()) {
            set_error("missing weight " + k);
            return nullptr;
        }
        if (numel >= 0 && it->second.second != numel) {
            set_error("weight " + k + " has " + std::to_string(it->second.second) + " elements, expected " +
                      std::to_string(numel));
            return nullptr;
        }
        return it->second.first;
    }
};

// The device blocks a handle owns for its whole life, each with 16 spare bytes at its end.
struct DeviceAllocs {
    std::vector<void*> ptrs;
    template <typename T>
    tts_status alloc(T** p, size_t n) {
        void* q = nullptr;
        TTS_HIP(hipMalloc(&q, n * sizeof(T) + 16));
        ptrs.push_back(q);
        *p = static_cast<T*>(q);
        return TTS_OK;
    }
    void free_all() {
        for (void* p : ptrs) (void)hipFree(p);
        ptrs.clear();
    }
};

// A grow-only device block of T.  reserve(need) keeps a block that holds `need` elements; else it
// frees it, allocates `need` and sets *moved.  The pointer is null and the capacity 0 between the
// two, so a failed hipMalloc leaves the owner destroyable.  What has to happen before a block may
// move (a stream still reading it) is the caller's: test cap first.
template <typename T>
struct DeviceBuf {
    T* p = nullptr;
    size_t cap = 0;
    tts_status reserve(size_t need, bool* moved = nullptr) {
        if (need <= cap) return TTS_OK;
        if (p) TTS_HIP(hipFree(p));
        p = nullptr;
        cap = 0;
        TTS_HIP(hipMalloc(&p, need * sizeof(T)));
        cap = need;
        if (moved) *moved = true;
        return TTS_OK;
    }
};

// A device copy of a checkpoint tensor in its reference layout.
inline tts_status copy_weight(DeviceAllocs& dev, float** dst, const float* src, size_t n, hipStream_t s) {
    TTS_TRY(dev.alloc(dst, n));
    TTS_HIP(hipMemcpyAsync(*dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    return TTS_OK;
}

// A [N][K] matrix / an N-row bias (a + b, b may be null) in the skinny GEMM's packed order (sgemm.h).
inline tts_status pack_linear(DeviceAllocs& dev, const float* W, int N, int K, float** dst, hipStream_t s) {
    TTS_TRY(dev.alloc(dst, sgemm_packed_floats(N, K)));
    TTS_HIP(sgemm_pack(W, K, nullptr, 0, N, ROWMAP_IDENTITY, 0, *dst, s));
    return TTS_OK;
}
inline tts_status pack_bias(DeviceAllocs& dev, const float* a, const float* b, int N, int rowmap, int H, float** dst,
                            hipStream_t s) {
    TTS_TRY(dev.alloc(dst, (size_t)(N + 15) / 16 * 16));
    TTS_HIP(sgemm_pack_bias(a, b, N, rowmap, H, *dst, s));
    return TTS_OK;
}

// The graphs of a multi-launch decoder for one (B, Lmax, max_steps): one even step, one odd step,
// and a chunk of steps starting even.  step(parity) enqueues one step on the capturing stream s.
struct StepGraphs {
    hipGraphExec_t step[2] = {nullptr, nullptr};
    hipGraphExec_t chunk = nullptr;
};

template <typename Step>
tts_status capture_steps(hipStream_t s, int first_parity, int steps, Step& step, hipGraphExec_t* out) {
    hipGraph_t g = nullptr;
    TTS_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    tts_status st = TTS_OK;
    for (int i = 0; i < steps && st == TTS_OK; ++i) st = step((first_parity + i) & 1);
    hipError_t e = hipStreamEndCapture(s, &g);
    if (st) return st;
    TTS_HIP(e);
    TTS_HIP(hipGraphInstantiate(out, g, nullptr, nullptr, 0));
    TTS_HIP(hipGraphDestroy(g));
    return TTS_OK;
}

template <typename Step>
tts_status build_step_graphs(StepGraphs& g, int chunk_len, hipStream_t s, Step step) {
    tts_status st = capture_steps(s, 0, 1, step, &g.step[0]);
    if (!st) st = capture_steps(s, 1, 1, step, &g.step[1]);
    if (!st) st = capture_steps(s, 0, chunk_len, step, &g.chunk);
    return st;
}

// Enqueues n steps after the `run` already enqueued: whole chunks from an even step, else single steps.
inline tts_status launch_steps(const StepGraphs& g, int chunk_len, int& run, int n, hipStream_t s) {
    while (n > 0) {
        if ((run & 1) == 0 && n >= chunk_len) {
            TTS_HIP(hipGraphLaunch(g.chunk, s));
            run += chunk_len;
            n -= chunk_len;
        } else {
            TTS_HIP(hipGraphLaunch(g.step[run & 1], s));
            ++run;
            --n;
        }
    }
    return TTS_OK;
}

inline void destroy_step_graphs(const StepGraphs& g) {
    for (hipGraphExec_t x : {g.step[0], g.step[1], g.chunk})
        if (x) (void)hipGraphExecDestroy(x);
}

// env_is: the variable is set and its first character is c ('\0': set and empty).
// env_int: atoi of the variable, dflt when it is unset.
inline bool env_is(const char* name, char c) {
    const char* v = std::getenv(name);
    return v && v[0] == c;
}
inline int env_int(const char* name, int dflt) {
    const char* v = std::getenv(name);
    return v ? std::atoi(v) : dflt;
}

}  // namespace tts
