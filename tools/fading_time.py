"""What block fading costs next to the AWGN calls of the same commit on the same inputs, one session on one card:
  (d) bldpc_qam_demap_fading against bldpc_qam_demap_il;
  (c) nbldpc_fading_channel_device_qam_frames against nbldpc_awgn_channel_device_qam_frames;
  (b) bldpc_awgn_fading_channel_device against bldpc_awgn_channel_device;
  (a) bldpc_fading_gains_device alone, at fast fading, Lc = 16 and one block per frame;
  (s) one sweep point, Simulation_GPU on J4_L24_Z96 over 64-QAM with the row-column interleaver, with and without fading.
(a) to (d) on J4_L24_Z96 with 65 536 frames and PON_LDPC (J12_L69_Z256) with 4 096; 64- and 256-QAM; both index rules.  Whole calls of
the C ABI between HIP events on the stream after warm-up, every output preallocated, the variants alternating inside every repetition;
median [min .. max].
usage: python tools/fading_time.py [--reps R] [--out FILE]   (GPU box)"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cuda_ldpc_amd as C  # noqa: E402
from cuda_ldpc_amd import nbldpc as nb  # noqa: E402
from cuda_ldpc_amd._lib import check, lib  # noqa: E402
from cuda_ldpc_amd.simulation import Simulation_GPU  # noqa: E402
from harq_time import timed_round  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 7:
        ap.error("at least 7 repetitions")
    if not torch.cuda.is_available():
        sys.exit("fading_time.py needs a GPU")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# python tools/fading_time.py --reps %d" % args.reps)
    emit("# %s, %d repetitions, C-ABI calls on preallocated outputs, alternating; ms = median [min .. max]; ratio = fading / AWGN" % (
        torch.cuda.get_device_name(0), args.reps))
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    NP = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    sigma, scale = ctypes.c_float(0.1), ctypes.c_float(1.0 / (2 * 0.1 * 0.1))
    cons = {q: torch.from_numpy(C.Get_CONSTELLATION(os.path.join(ROOT, "data", "nb", "Constellation", "GRAY_%dQAM.txt" % q), q)).cuda()
            for q in (64, 256)}
    seed = lambda: np.array([173, 173, 173], np.int32)  # noqa: E731  -- a call advances its host copy; the kernel's work does not depend on it

    def nb_check(rc, what):
        if rc != 0:
            raise RuntimeError("%s failed: %s" % (what, lib.nbldpc_last_error().decode(errors="replace")))

    def report(label, t, fad, awgn):
        med = {k: float(np.median(v)) for k, v in t.items()}
        fmt = lambda k: "%8.3f [%6.3f .. %6.3f]" % (med[k], min(t[k]), max(t[k]))  # noqa: E731
        emit("  %-34s %24s %24s %8.3f" % (label, fmt(fad), fmt(awgn), med[fad] / med[awgn]))
        return med[fad] / med[awgn]

    worst = {}
    for name, L, Z, F in (("J4_L24_Z96", 24, 96, 65536), ("PON_LDPC", 69, 256, 4096)):
        N = L * Z
        g = torch.Generator(device="cuda").manual_seed(N)
        emit("# %s N=%d F=%d" % (name, N, F))
        emit("# %-34s %24s %24s %8s" % ("call", "fading ms", "AWGN ms", "ratio"))
        # (b) and (a) over BPSK: S = N uses per frame
        gain = torch.empty((F, N), device="cuda")
        cw = torch.randint(0, 2, (N, F), generator=g, device="cuda", dtype=torch.int32)
        y1, y2 = torch.empty((N, F), device="cuda"), torch.empty((N, F), device="cuda")
        check(lib.bldpc_fading_gains_device(NP(seed()), 16, N, F, P(gain), st), "gains")
        fns = {"fading": lambda: check(lib.bldpc_awgn_fading_channel_device(NP(seed()), sigma, P(gain), P(y1), P(cw), N, F, st), "fading channel"),
               "awgn": lambda: check(lib.bldpc_awgn_channel_device(NP(seed()), sigma, P(y2), P(cw), N, F, st), "channel")}
        for Lc in (1, 16, N):
            fns["gains Lc=%d" % Lc] = lambda Lc=Lc: check(lib.bldpc_fading_gains_device(NP(seed()), Lc, N, F, P(gain), st), "gains")
        for f in fns.values():
            for _ in range(2):
                f()
        torch.cuda.synchronize()
        t = timed_round(fns, args.reps)
        report("(b) BPSK channel", t, "fading", "awgn")
        for Lc in (1, 16, N):
            k = "gains Lc=%d" % Lc
            emit("  %-34s %8.3f [%6.3f .. %6.3f]   (a) S=%d uses per frame, alone" % (k, float(np.median(t[k])), min(t[k]), max(t[k]), N))
        del gain, cw, y1, y2
        for q, con in cons.items():
            m = q.bit_length() - 1
            Ns = (N + m - 1) // m
            sym = torch.randint(0, q, (F, Ns), generator=g, device="cuda", dtype=torch.int32)
            gain = torch.empty((F, Ns), device="cuda")
            check(lib.bldpc_fading_gains_device(NP(seed()), 16, Ns, F, P(gain), st), "gains")
            rx1, rx2 = torch.empty((F, Ns, 2), device="cuda"), torch.empty((F, Ns, 2), device="cuda")
            o1, o2 = torch.empty((N, F), device="cuda"), torch.empty((N, F), device="cuda")
            fns = {"ch fading": lambda: nb_check(lib.nbldpc_fading_channel_device_qam_frames(NP(seed()), sigma, P(sym), Ns, P(con), q, P(gain), F,
                                                                                              P(rx1), st), "fading qam channel"),
                   "ch awgn": lambda: nb_check(lib.nbldpc_awgn_channel_device_qam_frames(NP(seed()), sigma, P(sym), Ns, P(con), q, F, P(rx2), st),
                                               "qam channel")}
            for il, rule in ((C.IL_NONE, "none"), (C.IL_ROWCOL, "rowcol")):
                fns["demap fading " + rule] = lambda il=il: check(lib.bldpc_qam_demap_fading(P(rx1), P(gain), P(con), q, scale, N, F, il, P(o1), st),
                                                                  "demap fading")
                fns["demap awgn " + rule] = lambda il=il: check(lib.bldpc_qam_demap_il(P(rx1), P(con), q, scale, N, F, il, P(o2), st), "demap")
            for f in fns.values():
                for _ in range(2):
                    f()
            torch.cuda.synchronize()
            t = timed_round(fns, args.reps)
            report("(c) %d-QAM channel" % q, t, "ch fading", "ch awgn")
            for rule in ("none", "rowcol"):
                r = report("(d) %d-QAM demapper, rule %s" % (q, rule), t, "demap fading " + rule, "demap awgn " + rule)
                worst[m] = max(worst.get(m, 0.0), r)
            del sym, gain, rx1, rx2, o1, o2
    for m, r in sorted(worst.items()):
        emit("# (d) the largest ratio of medians at M = %d: %.3f" % (m, r))

    # (s) one sweep point with and without fading; wall time of the whole call, counters read back included
    code = C.BinaryCode.from_blockh(os.path.join(ROOT, "data", "bldpc", "J4_L24_Z96_BlockH.txt"), 4, 24, 96)
    F, batches = 65536, 2
    con64 = cons[64].cpu().numpy()
    kw = dict(Num_Frames_OneTime=F, max_batches=batches, log=None, leastTestFrames=10 ** 12, device_channel=True, PN_Message=1, pn_seed=1, alpha=0.75,
              maxIT=25, exit_mode=C.EXIT_PER_FRAME, schedule="layered", n_QAM=64, CONSTELLATION=con64, interleave=C.IL_ROWCOL)
    points = {"AWGN, Eb/N0 11.0 dB": (nb.sigma_of(11.0, code.K / code.N, 0, 64), None),
              "fading Lc=16, Eb/N0 20.0 dB": (nb.sigma_of(20.0, code.K / code.N, 0, 64), 16)}
    times, sims = {k: [] for k in points}, {}
    for rep in range(args.reps + 2):
        for k, (sg, Lc) in points.items():
            SIM = C.SimCounters()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            Simulation_GPU(code, np.array([173, 173, 173], np.int32), sg, SIM, fading=None if Lc is None else C.Fading(Lc), **kw)
            torch.cuda.synchronize()
            if rep >= 2:  # two warm-up rounds
                times[k].append((time.perf_counter() - t0) * 1e3)
            sims[k] = SIM
    emit("# (s) Simulation_GPU, J4_L24_Z96 over 64-QAM rowcol, layered alpha 0.75, 25 iterations per-frame exit, random codewords, %d batches of "
         "%d frames; wall ms of the call, %d repetitions" % (batches, F, args.reps))
    for k, v in times.items():
        S = sims[k]
        emit("  %-30s %9.2f [%8.2f .. %8.2f]   error frames %d of %d, iterations per frame %.2f" % (
            k, float(np.median(v)), min(v), max(v), S.num_Error_Frames, S.num_Frames, S.Total_Iteration / max(S.num_Frames, 1)))
    ks = list(points)
    emit("  fading / AWGN = %.3f (the decoder's iterations differ with the operating point: see the counts)" % (
        float(np.median(times[ks[1]])) / float(np.median(times[ks[0]]))))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
