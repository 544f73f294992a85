"""Times of erasure decoding by elimination after peeling, one session on one card.
For J4_L24_Z96 at p = 0.12, 0.14 and 0.16 and J32_L64_Z64 at 0.42 with 65 536 frames, and PON at 0.14 with 4 096 frames, on the all-zero
word through the binary erasure channel from seed (173, 173, 173): bldpc_decode_erasure (100 iterations, Dbits + Ebits), then
bldpc_decode_erasure_ml on the first N rows of its Dbits and its Ebits (max_erased 0 = M, tier auto, Dbits + Ebits + status + rank).
Per row: the frames peeling leaves, the frames the list pass takes (status neither NONE nor SKIPPED), the frames left after
elimination, the milliseconds of both calls and of the new call per listed frame.  The yardstick is what a user has today for the same
task: bldpc_decode_erasure_ml_host, at most 16 threads, over the same words, timed once with the host clock (its copies not counted).
Whole C-ABI calls between HIP events on the stream, outputs preallocated, after warm-up; median, min and max over the repetitions
(15, fewer where one call takes more than 1.5 s).
usage: python tools/erasure_ml_time.py [--reps R] [--out FILE] [--no-host]   (GPU box)"""
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
CODES = (  # file, J, L, Z, frames, erasure probabilities
    ("J4_L24_Z96_BlockH.txt", 4, 24, 96, 65536, (0.12, 0.14, 0.16)),
    ("J32_L64_Z64_BlockH.txt", 32, 64, 64, 65536, (0.42,)),
    ("PON_LDPC.txt", 12, 69, 256, 4096, (0.14,)),
)
ITERS = 100


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def nptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def timed(fn, reps):
    ms = []
    for _ in range(reps):
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
        sys.exit("erasure_ml_time.py needs a GPU")
    out = None
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        out = open(args.out, "w")

    def emit(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    emit("# %s; ms = median [min .. max] of whole C-ABI calls between events; peeling capped at %d iterations; host: "
         "bldpc_decode_erasure_ml_host on %d threads" % (torch.cuda.get_device_name(0), ITERS, min(16, len(os.sched_getaffinity(0)))))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for fn, J, L, Z, F, ps in CODES:
        path = os.path.join(ROOT, "data", "bldpc", fn)
        code = C.BinaryCode.from_blockh(path, J, L, Z)
        H, _, _ = C.Get_H(path, J, L)
        name = fn.replace("_BlockH.txt", "").replace(".txt", "")
        N, W = code.N, (F + 31) // 32
        Db, Eb = (torch.empty((N + 1, W), dtype=torch.int32, device="cuda") for _ in range(2))
        Mb = torch.empty((N + 1, W), dtype=torch.int32, device="cuda")
        Me = torch.empty((N, W), dtype=torch.int32, device="cuda")
        it, status, rank = (torch.empty(F, dtype=torch.int32, device="cuda") for _ in range(3))
        emit("# %s N=%d M=%d F=%d, k_er_ml: %r" % (name, N, J * Z, F, code.erasure_ml_info()))
        emit("# %-12s %5s %-11s %5s %9s %8s %8s %26s %28s %10s %12s" % ("code", "p", "kernel", "reps", "peel left", "listed", "ml left", "peeling ms",
                                                                    "elimination ms", "ms/listed", "host ms"))
        for p in ps:
            bits, erased = C.BECChannel_GPU(np.array([173, 173, 173], np.int32), p, N, F)

            def peel():
                return lib.bldpc_decode_erasure(code._h, ptr(bits), ptr(erased), F, ITERS, None, ptr(Db), ptr(Eb), ptr(it), st)

            def ml():
                return lib.bldpc_decode_erasure_ml(code._h, ptr(Db), ptr(Eb), F, 0, 0, None, ptr(Mb), ptr(Me), ptr(status), ptr(rank), st)

            for _ in range(2):  # warm-up: plans, scratch growth
                assert peel() == 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            assert ml() == 0
            torch.cuda.synchronize()
            first = time.perf_counter() - t0
            assert ml() == 0
            reps = args.reps if first < 1.5 else max(3, min(args.reps, int(20.0 / first)))
            t_peel, t_ml = timed(peel, args.reps), timed(ml, reps)
            s = status.cpu().numpy()
            listed = int(((s != C.ML_NONE) & (s != C.ML_SKIPPED)).sum())
            flags_peel = C.Hard_Unpack(Db[N:].contiguous(), F).cpu().numpy()
            flags_ml = C.Hard_Unpack(Mb[N:].contiguous(), F).cpu().numpy()
            host = float("nan")
            if not args.no_host:
                hb, he = Db[:N].cpu().numpy().view(np.uint32), Eb.cpu().numpy().view(np.uint32)
                hD, hE, hs = np.zeros((N + 1, W), np.uint32), np.zeros((N, W), np.uint32), np.zeros(F, np.int32)
                Hh = np.ascontiguousarray(H, np.int32)
                t0 = time.perf_counter()
                rc = lib.bldpc_decode_erasure_ml_host(J, L, Z, nptr(Hh), nptr(np.ascontiguousarray(hb)), nptr(he), F, 0, None, nptr(hD), nptr(hE),
                                                      nptr(hs), None)
                host = (time.perf_counter() - t0) * 1e3
                assert rc == 0 and np.array_equal(hD, Mb.cpu().numpy().view(np.uint32)) and np.array_equal(hs, s)
                assert np.array_equal(hE, Me.cpu().numpy().view(np.uint32))
            emit("  %-12s %5g %-11s %5d %9d %8d %8d %9.3f [%6.3f .. %6.3f] %10.3f [%7.3f .. %7.3f] %10.5f %12.1f" % (
                name, p, code.last_kernel, reps, int((flags_peel == 0).sum()), listed, int((flags_ml == 0).sum()), *t_peel, *t_ml,
                t_ml[0] / max(listed, 1), host))
        code.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
