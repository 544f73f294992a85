"""Cost of encoding against decoding: per code, the time of bldpc_encode_random (messages generated on the device),
of bldpc_encode (messages read from memory), of bldpc_syndrome, and of the 50-iteration fixed decode of the same batch
(HIP events, median of the timed repetitions, after warm-up; the generator is built before timing and reported apart).
usage: python tools/encode_time.py [--reps R]   (GPU box)"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cuda_ldpc_amd as C  # noqa: E402

CODES = (  # file, J, L, Z, frames per batch (bench.py's where it has the code), Es/N0 dB
    ("J4_L24_Z96_BlockH.txt", 4, 24, 96, 65536, 3.0),
    ("J32_L64_Z64_BlockH.txt", 32, 64, 64, 32768, 0.0),
    ("J24_L60_Z160_BlockH.txt", 24, 60, 160, 16384, 2.0),
    ("J48_L60_Z160_BlockH.txt", 48, 60, 160, 16384, 2.0),
    ("PON_LDPC.txt", 12, 69, 256, 8192, 2.0),
    ("J15_L30_Z1280_BlockH.txt", 15, 30, 1280, 1024, 0.0),
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
    print("# %-24s %6s %6s %6s %8s | %9s %9s %9s %9s | %7s %7s | %9s %9s" % (
        "code", "F", "K'", "rank", "gen_s", "encR_ms", "enc_ms", "synd_ms", "dec_ms", "encR/dec", "enc/dec", "encR_Mcw/s", "dec_Mcw/s"))
    for fn, J, L, Z, F, snr in CODES:
        code = C.BinaryCode.from_blockh(os.path.join(ROOT, "data", "bldpc", fn), J, L, Z)
        t = time.time()
        K = code.K_info
        gen_s = time.time() - t
        cw, msg = C.PN_CodeWords(code, 1, F, want_msg=True)
        seed = np.array([173, 173, 173], np.int32)
        y = C.AWGNChannel_GPU(seed, C.sigma_of(snr), code.N, F, CodeWord=cw)
        D = torch.empty((code.N + 1, F), dtype=torch.int32, device="cuda")
        enc_r = lambda: C.PN_CodeWords(code, 1, F, CodeWord=cw)  # noqa: E731
        enc = lambda: C.Encode(code, msg, CodeWord=cw)  # noqa: E731
        syn = lambda: C.Syndrome(code, D)  # noqa: E731
        dec = lambda: C.LDPC_Decoder_GPU(code, y, max_iter=50, exit_mode=C.EXIT_FIXED, D=D)  # noqa: E731
        for f in (enc_r, enc, dec, syn):  # warm-up
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        t_er, t_e = timed(enc_r, args.reps), timed(enc, args.reps)
        t_d = timed(dec, max(3, args.reps // 4))
        t_s = timed(syn, args.reps)
        print("  %-24s %6d %6d %6d %8.2f | %9.4f %9.4f %9.4f %9.3f | %6.2f%% %6.2f%% | %9.2f %9.3f" % (
            fn.replace("_BlockH.txt", "").replace(".txt", ""), F, K, code.rank, gen_s, t_er, t_e, t_s, t_d, 100 * t_er / t_d,
            100 * t_e / t_d, F / t_er / 1e3, F / t_d / 1e3), flush=True)
        code.close()


if __name__ == "__main__":
    main()
