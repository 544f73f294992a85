"""Where the time of the fused channel + combine (bldpc_rm_awgn_combine_device) goes under a done mask: the same call with no frame
done, either half of the batch done, every other workgroup of 256 frames done, every other wavefront of 64 done and every frame done, at
several (N, F); no lists, k0 = N / 3, E = N, the all-zero word.  Median of 15 calls between HIP events after warm-up.  The figures
behind DESIGN 4.14 (a): a done pattern with a short period in workgroups saves nothing.
usage: python tools/harq_done_patterns.py [--out FILE]   (GPU box)"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cuda_ldpc_amd as C  # noqa: E402
from cuda_ldpc_amd._lib import check, lib  # noqa: E402


def median_ms(fn, reps=15):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("harq_done_patterns.py needs a GPU")
    lines = ["# python tools/harq_done_patterns.py: %s, bldpc_rm_awgn_combine_device, median of 15" % torch.cuda.get_device_name(0)]
    print(lines[0], flush=True)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    sigma, llr = ctypes.c_float(0.7), ctypes.c_float(1.0e4)
    seed = np.array([173, 173, 173], np.int32)
    sp = seed.ctypes.data_as(ctypes.c_void_p)
    for N, F in ((17664, 4096), (17664, 16384), (2304, 4096), (2304, 16384), (17664, 65536)):
        rm = C.RateMatch.circular(N, (), (), N // 3, N)
        acc = torch.zeros((N, F), device="cuda")
        pats = {k: torch.zeros(F, dtype=torch.int32) for k in ("none", "first half", "second half", "every other block of 256", "every other wave of 64")}
        pats["all"] = torch.ones(F, dtype=torch.int32)
        pats["first half"][:F // 2] = 1
        pats["second half"][F // 2:] = 1
        pats["every other block of 256"].view(-1, 256)[0::2] = 1
        pats["every other wave of 64"].view(-1, 64)[0::2] = 1
        base = None
        for k, d in pats.items():
            d = d.cuda()
            ms = median_ms(lambda: check(lib.bldpc_rm_awgn_combine_device(rm._h, sp, sigma, None, F, llr, P(d), P(acc), st), "fused"))
            base = base or ms
            lines.append("N=%d F=%d blocks=%d  %-26s %.3f ms  %.3f of none" % (N, F, (F // 256) * ((N + 31) // 32), k, ms, ms / base))
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
