"""Cost of encoding against decoding for the GF(q) codes: per shipped matrix, the generator build time (host, first use), and the time
of nbldpc_encode_random (messages generated on the device), nbldpc_encode (messages read from memory), nbldpc_syndrome, the per-frame
device channel, and the EMS(2,2) decode (maxIT 20) of the same batch (HIP events, median of the timed repetitions, after warm-up).
usage: python tools/nb_encode_time.py [--reps R]   (GPU box)"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cuda_ldpc_amd import nbldpc as nb  # noqa: E402

NB = os.path.join(ROOT, "data", "nb")
CODES = (  # file, frames per batch (bench.py's where it has the code), Eb/N0 dB of the decode
    ("BDS.576.288.GF.64.txt", 16384, 3.0),
    ("LDPC_N576_K288_GF64_d1_exp.txt", 16384, 3.0),
    ("LDPC_N96_K48_GF256_d1_exp.txt", 8192, 4.0),
    ("LDPC_N576_K480_GF256_exp.txt", 1024, 5.0),
    ("Tanner_74_9_Z128_GF16.txt", 256, 5.0),
)


def timed(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    print("# %-30s %6s %5s %5s %7s | %9s %9s %9s %9s %9s | %8s" % (
        "code", "B", "K'", "rank", "gen_s", "encR_ms", "enc_ms", "synd_ms", "chan_ms", "dec_ms", "encR/dec"))
    for fn, B, snr in CODES:
        q = int(open(os.path.join(NB, fn)).readline().split()[2])
        mul, _, _ = nb.GFInitial(q, os.path.join(NB, "GF", "Arith.Table.GF.%d.txt" % q))
        code = nb.NBCode(os.path.join(NB, fn), mul)
        t = time.time()
        K = code.K_info
        gen_s = time.time() - t
        cw, msg = nb.PN_CodeWords(code, 1, B, want_msg=True)
        sigma = nb.sigma_of(snr, code.rate)
        seed = np.array([173, 173, 173], np.int32)
        Lch = nb.Demodulate(code, nb.AWGNChannel_GPU(seed, sigma, code, cw, B), sigma)
        out = torch.empty((B, code.N), dtype=torch.int32, device="cuda")
        enc_r = lambda: nb.PN_CodeWords(code, 1, B, CodeWord_sym=cw)  # noqa: E731
        enc = lambda: nb.Encode(code, msg, CodeWord_sym=cw)  # noqa: E731
        syn = lambda: nb.Syndrome(code, out)  # noqa: E731
        chan = lambda: nb.AWGNChannel_GPU(seed, sigma, code, cw, B)  # noqa: E731
        dec = lambda: nb.Decoding_EMS(code, Lch, 2, 2, 20)  # noqa: E731
        for f in (enc_r, enc, syn, chan, dec):  # warm-up
            for _ in range(2):
                f()
        torch.cuda.synchronize()
        t_er, t_e, t_s, t_c = timed(enc_r, args.reps), timed(enc, args.reps), timed(syn, args.reps), timed(chan, args.reps)
        t_d = timed(dec, max(3, args.reps // 4))
        print("  %-30s %6d %5d %5d %7.3f | %9.4f %9.4f %9.4f %9.4f %9.3f | %7.2f%%" % (
            fn.replace(".txt", ""), B, K, code.rank, gen_s, t_er, t_e, t_s, t_c, t_d, 100 * t_er / t_d), flush=True)
        code.close()


if __name__ == "__main__":
    main()
