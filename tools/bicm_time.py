"""What the QAM path of the binary sweep costs next to what it feeds, one session on one card: J4_L24_Z96, 65 536 frames,
64-QAM and 256-QAM (Constellation/GRAY_<q>QAM.txt), random codewords.
  map      bldpc_qam_map            codeword bits [N][F] -> constellation indices [F][Ns]
  channel  nbldpc_awgn_channel_device_qam_frames   (four RandomModule draws, two logf/sqrtf/cos per symbol)
  demap    bldpc_qam_demap          received points -> max-log soft values [N][F]
and, in the same session, the BPSK channel generator (bldpc_awgn_channel_device, 2 draws and one logf/sqrtf/sin per BIT) and the
50-iteration fixed flooding decode of the same batch.  Whole calls of the C ABI between HIP events on the stream after warm-up, every
output preallocated (no call allocates), the calls alternating inside every repetition; median [min .. max] over the repetitions.
"GB/s moved" is input plus output bytes over the time: it says how near a call is to a copy, and is left out for the decode, whose
50 iterations run on-chip.
usage: python tools/bicm_time.py [--reps R] [--frames F] [--out FILE]   (GPU box)"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cuda_ldpc_amd as C  # noqa: E402
from cuda_ldpc_amd import nbldpc as nb  # noqa: E402
from cuda_ldpc_amd._lib import check, lib  # noqa: E402


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
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--frames", type=int, default=65536)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 7:
        ap.error("at least 7 repetitions")
    if not torch.cuda.is_available():
        sys.exit("bicm_time.py needs a GPU")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    J, L, Z, F = 4, 24, 96, args.frames
    code = C.BinaryCode.from_blockh(os.path.join(ROOT, "data", "bldpc", "J4_L24_Z96_BlockH.txt"), J, L, Z)
    N = code.N
    emit("# %s, J4_L24_Z96 N=%d, F=%d frames, %d repetitions, C-ABI calls on preallocated outputs, alternating; ms = median [min .. max]" % (
        torch.cuda.get_device_name(0), N, F, args.reps))
    emit("# %-8s %-34s %22s %10s %12s" % ("q", "call", "ms", "Mframes/s", "GB/s moved"))
    cw = C.PN_CodeWords(code, 1, F)
    D = torch.empty((N + 1, F), dtype=torch.int32, device="cuda")
    for q in (64, 256):
        m = q.bit_length() - 1
        Ns = (N + m - 1) // m
        con = torch.from_numpy(C.Get_CONSTELLATION(os.path.join(ROOT, "data", "nb", "Constellation", "GRAY_%dQAM.txt" % q), q)).cuda()
        sigma = nb.sigma_of(12.0, code.K / N, 0, q)
        sym = C.Modulate_QAM(cw, N, m)
        rx = C.AWGNChannel_QAM_GPU(np.array([173, 173, 173], np.int32), sigma, sym, con)
        y = C.Demodulate_QAM(rx, con, 1.0 / (2 * sigma * sigma), N)
        seed = np.array([173, 173, 173], np.int32)
        # the C ABI on preallocated outputs, as a C caller would use it: the Python wrappers allocate their result
        scale = ctypes.c_float(1.0 / (2 * sigma * sigma))
        sym_o, rx_o, y_o, yb_o = torch.empty_like(sym), torch.empty_like(rx), torch.empty_like(y), torch.empty_like(y)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        sp = seed.ctypes.data_as(ctypes.c_void_p)
        it = ctypes.c_int(0)
        fns = {
            "map": lambda: check(lib.bldpc_qam_map(P(cw), N, F, m, P(sym_o), st), "map"),
            "QAM channel": lambda: nb._check(lib.nbldpc_awgn_channel_device_qam_frames(sp, ctypes.c_float(sigma), P(sym), Ns, P(con), q, F, P(rx_o), st),
                                             "QAM channel"),
            "demap": lambda: check(lib.bldpc_qam_demap(P(rx), P(con), q, scale, N, F, P(y_o), st), "demap"),
            "BPSK channel (bldpc_awgn_channel_device)": lambda: check(lib.bldpc_awgn_channel_device(sp, ctypes.c_float(sigma), P(yb_o), P(cw), N, F, st),
                                                                      "BPSK channel"),
            "flooding decode, 50 fixed": lambda: check(lib.bldpc_decode(code._h, P(y), F, 50, 0, C.EXIT_FIXED, C.KERNEL_AUTO, P(D), None, None,
                                                                        ctypes.byref(it), st), "decode"),
        }
        moved = {  # bytes read + written by the call
            "map": 4 * N * F + 4 * Ns * F, "QAM channel": 4 * Ns * F + 8 * Ns * F, "demap": 8 * Ns * F + 4 * N * F,
            "BPSK channel (bldpc_awgn_channel_device)": 8 * N * F, "flooding decode, 50 fixed": 0,
        }
        for f in fns.values():
            for _ in range(2):
                f()
        torch.cuda.synchronize()
        t = timed_round(fns, args.reps)
        med = {k: float(np.median(v)) for k, v in t.items()}
        for k in fns:
            emit("  %-8d %-34s %8.3f [%6.3f .. %6.3f] %10.2f %12s" % (q, k[:34], med[k], min(t[k]), max(t[k]), F / med[k] / 1e3,
                                                                    "%.1f" % (moved[k] / med[k] / 1e6) if moved[k] else "-"))
        emit("  %-8d demap / BPSK channel = %.2f;  (map + demap) / decode = %.3f;  (map + QAM channel + demap) / decode = %.3f" % (
            q, med["demap"] / med["BPSK channel (bldpc_awgn_channel_device)"], (med["map"] + med["demap"]) / med["flooding decode, 50 fixed"],
            (med["map"] + med["QAM channel"] + med["demap"]) / med["flooding decode, 50 fixed"]))
    code.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
