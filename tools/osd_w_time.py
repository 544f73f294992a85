"""Times of reprocessing of order 0, 1 and 2 after a layered decode, one session on one card.
The inputs are those of tools/osd_time.py: J4_L24_Z96 (65 536 frames, LDS tier) and J32_L64_Z64 (4 096 frames, workspace tier) on the
all-zero word over the AWGN channel from seed (173, 173, 173), bldpc_decode_layered (ten iterations, alpha 0.75, per-frame exit,
syndrome rule, with app), then reprocessing in place on its D and app (tier auto, every output).  Per noise level one row per call:
bldpc_decode_osd, then bldpc_decode_osd_w at order 0, order 1 and order 2 with lambda 16 and 60; per row the frames on the list, the
frames in error after the call, the milliseconds of the call and per listed frame, and beside it bldpc_decode_osd_w_host (at most 16
threads) over the same inputs, timed once with the host clock and held to the kernel's outputs.  The first two rows are the timing
condition of order 0: the kernels of bldpc_decode_osd are the ones of the commit before, instruction for instruction, and order 0
through the new entry point has to lie within the spread of the repetitions of the two; the tool says so in a line of its own.
Whole C-ABI calls between HIP events on the stream, outputs preallocated, after warm-up; the flag row is put back before every
repetition, outside the events; median, min and max over the repetitions (15, fewer where one call takes more than 1.5 s).
usage: python tools/osd_w_time.py [--reps R] [--out FILE] [--no-host]   (GPU box)"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cuda_ldpc_amd as C  # noqa: E402
from tools.osd_time import ALPHA, CODES, ITERS, nptr, ptr, timed  # noqa: E402

lib = C._lib.lib
SETS = ((None, 0), (0, 0), (1, 0), (2, 16), (2, 60))  # (order, lambda); None: bldpc_decode_osd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("osd_w_time.py needs a GPU")
    out = None
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        out = open(args.out, "w")

    def emit(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    emit("# %s; measured on the GPU: ms = median [min .. max] of whole C-ABI calls between events; layered min-sum, %d iterations, alpha %g, "
         "per-frame exit, syndrome rule; host: bldpc_decode_osd_w_host on %d threads, host clock, once"
         % (torch.cuda.get_device_name(0), ITERS, ALPHA, min(16, len(os.sched_getaffinity(0)))))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for fn, J, L, Z, F, sigmas in CODES:
        path = os.path.join(ROOT, "data", "bldpc", fn)
        code = C.BinaryCode.from_blockh(path, J, L, Z)
        H, _, _ = C.Get_H(path, J, L)
        Hh = np.ascontiguousarray(H, np.int32)
        name = fn.replace("_BlockH.txt", "").replace(".txt", "")
        N = code.N
        D = torch.empty((N + 1, F), dtype=torch.int32, device="cuda")
        app = torch.empty((N, F), dtype=torch.float32, device="cuda")
        it, flips, scanned = (torch.empty(F, dtype=torch.int32, device="cuda") for _ in range(3))
        picked = torch.empty((2, F), dtype=torch.int32, device="cuda")
        metric = torch.zeros(F, dtype=torch.float32, device="cuda")
        emit("# %s N=%d M=%d rank=%d F=%d, k_osd_w at order 2: %r" % (name, N, J * Z, N - code.K_info, F, code.osd_info(order=2)))
        emit("# %-12s %5s %-18s %-10s %5s %8s %9s %32s %10s %12s" % ("code", "sigma", "call", "kernel", "reps", "listed", "err after", "reprocessing ms",
                                                                  "ms/listed", "host ms"))
        for sigma in sigmas:
            y = C.AWGNChannel_GPU(np.array([173, 173, 173], np.int32), sigma, N, F)
            for _ in range(2):
                assert lib.bldpc_decode_layered(code._h, ptr(y), F, ITERS, ctypes.c_float(ALPHA), 0, C.EXIT_PER_FRAME, C.STOP_SYNDROME, ptr(D),
                                                ptr(app), ptr(it), st) == 0
            torch.cuda.synchronize()
            D0 = D.clone()
            listed = int((D0[N] == 0).sum())

            def put_back():
                D.copy_(D0)

            spread = {}
            for order, lam in SETS:
                if order is None:
                    def osd():
                        return lib.bldpc_decode_osd(code._h, ptr(app), ptr(D), F, 0, ptr(D), ptr(flips), ptr(scanned), st)
                else:
                    def osd(order=order, lam=lam):
                        return lib.bldpc_decode_osd_w(code._h, ptr(app), ptr(D), F, 0, order, lam, ptr(D), ptr(flips), ptr(scanned), ptr(picked),
                                                      ptr(metric), st)
                put_back()
                torch.cuda.synchronize()
                assert osd() == 0  # the first call builds the plan: the code's generator, for the rank
                torch.cuda.synchronize()
                put_back()
                t0 = time.perf_counter()
                assert osd() == 0
                torch.cuda.synchronize()
                first = time.perf_counter() - t0
                reps = args.reps if first < 1.5 else max(3, min(args.reps, int(20.0 / first)))
                t = timed(osd, reps, before=put_back)
                spread[order, lam] = t
                after = int((D[:N] != 0).any(0).sum())
                host = float("nan")
                if not args.no_host and order is not None:
                    ha, oD = app.cpu().numpy(), D0.cpu().numpy()  # in place, as the kernel: no kept frame is copied
                    of, osc, opk, om = np.zeros(F, np.int32), np.zeros(F, np.int32), np.zeros((2, F), np.int32), np.zeros(F, np.float32)
                    t0 = time.perf_counter()
                    rc = lib.bldpc_decode_osd_w_host(J, L, Z, nptr(Hh), nptr(ha), nptr(oD), F, order, lam, nptr(oD), nptr(of), nptr(osc), nptr(opk),
                                                     nptr(om))
                    host = (time.perf_counter() - t0) * 1e3
                    done = of >= 0
                    assert rc == 0 and np.array_equal(oD, D.cpu().numpy()) and np.array_equal(of, flips.cpu().numpy())
                    assert np.array_equal(osc, scanned.cpu().numpy()) and np.array_equal(opk, picked.cpu().numpy())
                    assert np.array_equal(om.view(np.uint32)[done], metric.cpu().numpy().view(np.uint32)[done])
                call = "bldpc_decode_osd" if order is None else "osd_w order %d lam %d" % (order, lam)
                emit("  %-12s %5g %-18s %-10s %5d %8d %9d %10.3f [%8.3f .. %9.3f] %10.5f %12.1f" % (
                    name, sigma, call, code.last_kernel, reps, listed, after, *t, t[0] / max(listed, 1), host))
            a, b = spread[None, 0], spread[0, 0]
            inside = a[1] <= b[0] <= a[2] or b[1] <= a[0] <= b[2]
            emit("# %s sigma %g: order 0 through bldpc_decode_osd_w, median %.3f ms, against bldpc_decode_osd, median %.3f ms: %s the spread of the "
                 "repetitions of the two" % (name, sigma, b[0], a[0], "within" if inside else "NOT within"))
        code.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
