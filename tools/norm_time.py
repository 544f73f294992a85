"""Normalised against plain flooding decode rates (and the layered decoder next to them), one session on one card, for the two
bench.py codes at bench.py's batch sizes:
  (a) plain flooding, 50 fixed iterations through bldpc_decode (LDPC_Decoder_GPU, kernel AUTO)
  (b) normalised flooding, 50 fixed iterations, alpha 0.75 (bldpc_decode_normalised; and alpha 1.0: the same kernel, the plain bits)
  (c) layered, 25 fixed iterations, alpha 0.75
  (d) the two flooding per-frame paths at Es/N0 3.0, 3.6 and 4.2 dB (max 50; the all-zero codeword is sent, as in bench.py), with
      the mean iteration count and the frames left unflagged.
Whole calls (input regrouping, kernel, unpacking of D) between HIP events on the stream, after warm-up; the variants alternate
inside every repetition; median, min and max over the repetitions are printed, the rate is frames / median.
usage: python tools/norm_time.py [--reps R] [--out FILE]   (GPU box)"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cuda_ldpc_amd as C  # noqa: E402

CODES = (  # file, J, L, Z, frames (bench.py), Es/N0 dB of the fixed-iteration workload (bench.py)
    ("J4_L24_Z96_BlockH.txt", 4, 24, 96, 65536, 3.0),
    ("J32_L64_Z64_BlockH.txt", 32, 64, 64, 32768, 0.0),
)
PF_SNR = {4: (3.0, 3.6, 4.2), 32: (3.0, 3.6, 4.2)}


def timed_round(fns, reps):
    """Every function once per repetition, in turn; returns {name: [ms per repetition]}."""
    out = {k: [] for k in fns}
    for _ in range(reps):
        ev = {}
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            ev[k] = (a, b)
        torch.cuda.synchronize()
        for k, (a, b) in ev.items():
            out[k].append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("norm_time.py needs a GPU")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# %s, %d repetitions, variants alternating; ms = median [min .. max] of whole calls; rate = frames / median" % (
        torch.cuda.get_device_name(0), args.reps))
    emit("# %-12s %6s %-34s %-14s %8s %22s %10s %8s %9s" % ("code", "F", "variant", "kernel", "Es/N0", "ms", "Mcw/s", "meanIT", "unflagged"))
    for fn, J, L, Z, F, snr in CODES:
        code = C.BinaryCode.from_blockh(os.path.join(ROOT, "data", "bldpc", fn), J, L, Z)
        name = fn.replace("_BlockH.txt", "")
        D = torch.empty((code.N + 1, F), dtype=torch.int32, device="cuda")

        def run(y, fns, info):
            for f in fns.values():  # warm-up: code objects, scratch growth
                for _ in range(2):
                    f()
            torch.cuda.synchronize()
            t = timed_round(fns, args.reps)
            for k in fns:
                fns[k]()
                kern = code.last_kernel
                r = info[k]()
                med = float(np.median(t[k]))
                emit("  %-12s %6d %-38s %-14s %8.1f %8.3f [%6.3f .. %6.3f] %10.3f %8.2f %9d" % (
                    name, F, k, kern, r[0], med, min(t[k]), max(t[k]), F / med / 1e3, r[1], r[2]))

        y = C.AWGNChannel_GPU(np.array([173, 173, 173], np.int32), C.sigma_of(snr), code.N, F)
        fixed = {
            "flooding 50 fixed": lambda: C.LDPC_Decoder_GPU(code, y, max_iter=50, exit_mode=C.EXIT_FIXED, D=D),
            "normalised 50 fixed alpha=0.75": lambda: C.LDPC_Decoder_GPU(code, y, max_iter=50, exit_mode=C.EXIT_FIXED, D=D, alpha=0.75),
            "normalised 50 fixed alpha=1.0": lambda: C.LDPC_Decoder_GPU(code, y, max_iter=50, exit_mode=C.EXIT_FIXED, D=D, alpha=1.0),
            "layered 25 fixed alpha=0.75": lambda: C.LDPC_Decoder_Layered_GPU(code, y, max_iter=25, alpha=0.75, D=D),
        }
        unfl = lambda: int((D[code.N] == 0).sum())  # noqa: E731
        run(y, fixed, {k: (lambda k=k: (snr, 25.0 if k.startswith("layered") else 50.0, unfl())) for k in fixed})
        for s in PF_SNR[J]:
            y = C.AWGNChannel_GPU(np.array([173, 173, 173], np.int32), C.sigma_of(s), code.N, F)
            last = {}

            def flood():
                last["it"] = C.LDPC_Decoder_GPU(code, y, max_iter=50, exit_mode=C.EXIT_PER_FRAME, D=D)["iters"]

            def norm():
                last["it"] = C.LDPC_Decoder_GPU(code, y, max_iter=50, exit_mode=C.EXIT_PER_FRAME, D=D, alpha=0.75)["iters"]

            inf = lambda s=s: (s, float(last["it"].float().mean()), unfl())  # noqa: E731
            run(y, {"flooding per-frame max 50": flood, "normalised per-frame max 50 alpha=0.75": norm},
                {"flooding per-frame max 50": inf, "normalised per-frame max 50 alpha=0.75": inf})
        code.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
