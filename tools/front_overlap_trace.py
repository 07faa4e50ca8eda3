"""From a rocprofv3 --kernel-trace run of pipelined configs[1] sentences (tools/b1_trace.py): for every
sentence k, when sentence k+1's encoder stage starts and ends relative to sentence k's
gl_persistent_kernel.  Measurement only:  python tools/front_overlap_trace.py <trace dir>

Per line (us, relative to the start of sentence k's Griffin-Lim loop): the loop's end, the next
sentence's first encoder-stage launch (stage_ids_kernel), its encoder_resident_kernel start and end,
and the next resident decoder's start.  Last line: in how many hand-overs the encoder stage started
before the loop ended, and the mean time the next decoder started after the loop's end."""
import csv
import glob
import sys


def main(d):
    kt = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)[0]
    rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(kt)))

    def of(name):
        return [r for r in rows if name in r[2]]

    gl, ids, enc, dec = of("gl_persistent_kernel"), of("stage_ids_kernel"), of("encoder_resident_kernel"), \
        of("resident_decoder_kernel")
    early, lag, n = 0, 0.0, 0
    for g in gl[2:]:  # (the first sentences: warm-up, code-object loads)
        # the next sentence: the first decoder launch after this loop began, the encoder launches before it
        nxt_dec = next((r for r in dec if r[0] > g[0]), None)
        nxt_enc = max((r for r in enc if nxt_dec and r[1] <= nxt_dec[0]), default=None)
        nxt_ids = max((r for r in ids if nxt_enc and r[0] < nxt_enc[0]), default=None)
        if not (nxt_ids and nxt_enc and nxt_dec):
            continue
        us = lambda t: (t - g[0]) / 1e3
        print(f"gl end {us(g[1]):8.1f}  next ids {us(nxt_ids[0]):8.1f}  next encoder_resident {us(nxt_enc[0]):8.1f} .. "
              f"{us(nxt_enc[1]):8.1f}  next decoder {us(nxt_dec[0]):8.1f}")
        n += 1
        early += nxt_ids[0] < g[1]
        lag += us(nxt_dec[0]) - us(g[1])
    print(f"encoder stage started before the Griffin-Lim loop ended in {early} of {n} hand-overs; "
          f"next decoder starts {lag / max(n, 1):.1f} us after the loop's end (mean)")


if __name__ == "__main__":
    main(sys.argv[1])
