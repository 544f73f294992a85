"""Times of ordered-statistics reprocessing after a layered decode, one session on one card.
For J4_L24_Z96 (65 536 frames, LDS tier) and J32_L64_Z64 (4 096 frames, workspace tier) on the all-zero word over the AWGN channel from
seed (173, 173, 173) at a few noise levels: bldpc_decode_layered (ten iterations, alpha 0.75, per-frame exit, syndrome rule, with app),
then bldpc_decode_osd in place on its D and app (tier auto, flips and scanned).  Per row: the frames the decoder leaves with a non-zero
syndrome (the frames the list pass takes), the frames in error before and after, the milliseconds of both calls and of the new call per
listed frame.  The yardstick is what a user has without the kernel: bldpc_decode_osd_host, at most 16 threads, over the same inputs,
in place as the kernel, timed once with the host clock (the copies from the card not counted) and held to the kernel's outputs.
Whole C-ABI calls between HIP events on the stream, outputs preallocated, after warm-up; the flag row is put back before every
repetition, outside the events; median, min and max over the repetitions (15, fewer where one call takes more than 1.5 s).
usage: python tools/osd_time.py [--reps R] [--out FILE] [--no-host]   (GPU box)"""
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

lib = C._lib.lib
CODES = (  # file, J, L, Z, frames, sigmas
    ("J4_L24_Z96_BlockH.txt", 4, 24, 96, 65536, (0.46, 0.50, 0.54)),
    ("J32_L64_Z64_BlockH.txt", 32, 64, 64, 4096, (0.80, 0.90)),
)
ITERS, ALPHA = 10, 0.75


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def nptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def timed(fn, reps, before=None):
    ms = []
    for _ in range(reps):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        assert fn() == 0
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("osd_time.py needs a GPU")
    out = None
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        out = open(args.out, "w")

    def emit(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    emit("# %s; ms = median [min .. max] of whole C-ABI calls between events; layered min-sum, %d iterations, alpha %g, per-frame exit, "
         "syndrome rule; host: bldpc_decode_osd_host on %d threads" % (torch.cuda.get_device_name(0), ITERS, ALPHA,
                                                                      min(16, len(os.sched_getaffinity(0)))))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for fn, J, L, Z, F, sigmas in CODES:
        path = os.path.join(ROOT, "data", "bldpc", fn)
        code = C.BinaryCode.from_blockh(path, J, L, Z)
        H, _, _ = C.Get_H(path, J, L)
        name = fn.replace("_BlockH.txt", "").replace(".txt", "")
        N = code.N
        D = torch.empty((N + 1, F), dtype=torch.int32, device="cuda")
        app = torch.empty((N, F), dtype=torch.float32, device="cuda")
        it, flips, scanned = (torch.empty(F, dtype=torch.int32, device="cuda") for _ in range(3))
        emit("# %s N=%d M=%d rank=%d F=%d, k_osd: %r" % (name, N, J * Z, N - code.K_info, F, code.osd_info()))
        emit("# %-12s %5s %-9s %5s %8s %10s %9s %26s %30s %10s %12s" % ("code", "sigma", "kernel", "reps", "listed", "err before", "err after",
                                                                     "layered ms", "reprocessing ms", "ms/listed", "host ms"))
        for sigma in sigmas:
            y = C.AWGNChannel_GPU(np.array([173, 173, 173], np.int32), sigma, N, F)

            def decode():
                return lib.bldpc_decode_layered(code._h, ptr(y), F, ITERS, ctypes.c_float(ALPHA), 0, C.EXIT_PER_FRAME, C.STOP_SYNDROME, ptr(D), ptr(app),
                                                ptr(it), st)

            def osd():
                return lib.bldpc_decode_osd(code._h, ptr(app), ptr(D), F, 0, ptr(D), ptr(flips), ptr(scanned), st)

            for _ in range(2):  # warm-up: plans, scratch growth
                assert decode() == 0
            t_dec = timed(decode, args.reps)
            D0 = D.clone()
            flag0 = D[N].clone()

            def put_back():
                D[N].copy_(flag0)

            torch.cuda.synchronize()
            assert osd() == 0  # the first call builds the plan: the code's generator, for the rank
            torch.cuda.synchronize()
            put_back()
            t0 = time.perf_counter()
            assert osd() == 0
            torch.cuda.synchronize()
            first = time.perf_counter() - t0
            reps = args.reps if first < 1.5 else max(3, min(args.reps, int(20.0 / first)))
            t_osd = timed(osd, reps, before=put_back)
            listed = int((flag0 == 0).sum())
            before = int(((flag0 == 0) | (D0[:N] != 0).any(0)).sum())
            after = int((D[:N] != 0).any(0).sum())
            host = float("nan")
            if not args.no_host:
                ha, oD = app.cpu().numpy(), D0.cpu().numpy()  # in place, as the kernel: no kept frame is copied
                of, osc = np.zeros(F, np.int32), np.zeros(F, np.int32)
                Hh = np.ascontiguousarray(H, np.int32)
                t0 = time.perf_counter()
                rc = lib.bldpc_decode_osd_host(J, L, Z, nptr(Hh), nptr(ha), nptr(oD), F, nptr(oD), nptr(of), nptr(osc))
                host = (time.perf_counter() - t0) * 1e3
                assert rc == 0 and np.array_equal(oD, D.cpu().numpy()) and np.array_equal(of, flips.cpu().numpy())
                assert np.array_equal(osc, scanned.cpu().numpy())
            emit("  %-12s %5g %-9s %5d %8d %10d %9d %9.3f [%6.3f .. %6.3f] %11.3f [%7.3f .. %8.3f] %10.5f %12.1f" % (
                name, sigma, code.last_kernel, reps, listed, before, after, *t_dec, *t_osd, t_osd[0] / max(listed, 1), host))
        code.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
