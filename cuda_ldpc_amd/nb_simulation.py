"""Simulation and Eb/N0 sweep of the reference's non-binary program, driven through the C ABI.

Mirrors myNBLDPC/src/Simulation.cpp:16-87 (decode_once_cpu: channel -> Demodulate -> Decoding_EMS -> Statistic until
`num_Error_Frames >= leastErrorFrames && num_Frames >= leastTestFrames`) and src/main.cu:215-260 (sweep: seeds reset
to 173/173/173 at every point, sigma from Eb/N0 and the code rate).  The reference decodes one frame per call and tests
its stop rule after every frame; here frames are decoded in batches, the per-frame results are then accounted in stream
order and the accounting stops at the frame at which the reference would have stopped, so the counters are the ones a
single-threaded reference run (THREAD_NUM 1) produces.
"""
import numpy as np
import torch

from . import nbldpc as nb
from . import sharding
from .bldpc import Fading, Fading_Gains


class _SeedsAfter:
    """seeds_before[b] of a device-generated batch, computed on demand by jump-ahead."""

    def __init__(self, seed0, code, qam=False):
        self.seed0, self.code, self.qam = seed0, code, qam

    def __getitem__(self, b):
        return nb.seed_after(self.seed0, b, self.code, self.qam)


class NBSim:
    """The counters of class Simulation (include/struct.h:52-71) that the NB program uses."""

    def __init__(self, SNR=0.0):
        self.SNR = SNR
        self.num_Frames = 0
        self.num_Error_Frames = 0
        self.num_Error_Bits = 0   # symbol errors (the reference's name, Simulation.cpp:276)
        self.Total_Iteration = 0

    def row(self, N):
        n = max(self.num_Frames, 1)
        # Simulation.cpp:193-198: FER, "BER" = symbol errors / frames / N, AverageIT
        return " %.1f %8d  %4d  %6.4e  %6.4e  %.2f" % (self.SNR, self.num_Frames, self.num_Error_Frames, self.num_Error_Frames / n,
                                                  self.num_Error_Bits / n / N, self.Total_Iteration / n)


def Simulation_GPU(code, seed, sigma, SIM, CodeWord_sym, EMS_Nm=2, EMS_Nc=2, maxIT=20, batch=1024, leastErrorFrames=50,
                   leastTestFrames=1000, max_frames=None, device=None, device_channel=False, decoder_method=0, CONSTELLATION=None,
                   PN_Message=0, pn_seed=0, fading=None):
    """One Eb/N0 point. `seed` (int32[3]) advances exactly as far as the reference would have drawn.
    device_channel: generate the noise on the GPU (same uniforms, device libm) instead of the host, frame by frame.
    decoder_method (define.h:37, Simulation.cpp:54-70): 0 EMS, 1 trellis min-max, 2 log-QSPA = EMS(q, dc-1), 3 layered TMM.
    CONSTELLATION (host float32 [q, 2], Get_CONSTELLATION): the n_QAM = q branches of Modulate / AWGNChannel_CPU / Demodulate
    (one constellation point per code symbol) instead of BPSK; the caller passes the sigma of that n_QAM.
    PN_Message=1: every frame sends its own random codeword in place of CodeWord_sym (may be None): frame i of the point is
    PN_CodeWords(code, pn_seed, ..., first_frame=i) (nbldpc_encode_random), and its errors are counted against that word.  The
    decoders stop on their own syndrome, so the stop rule and the seed roll-back are unchanged.
    fading (a Fading): flat Rayleigh block fading with receiver CSI over the QAM channel (include/nbldpc.h): every batch draws one gain
    per block of Lc symbols and frame from the fading stream, fading.seed (ceil(N / Lc) draws per frame; rolled back with the noise seed
    to the frame at which the reference would have stopped), sends the points through nbldpc_fading_channel_device_qam_frames -- one
    word for all frames is expanded to [batch, N] first, the draws are where the per-frame channel puts them -- and demodulates against
    the faded points (Demodulate_QAM_Fading).  Needs CONSTELLATION and device_channel=True."""
    if PN_Message not in (0, 1):
        raise ValueError("PN_Message must be 0 (CodeWord_sym for every frame) or 1 (random codewords)")
    if fading is not None:  # every refusal before anything touches the device
        if not isinstance(fading, Fading):
            raise ValueError("fading must be a Fading (block length and the seed of the fading stream), not %r" % (fading,))
        if not device_channel:
            raise ValueError("fading needs device_channel=True: the gains and the channel that applies them run on the device")
        if CONSTELLATION is None:
            raise ValueError("fading needs CONSTELLATION: the GF(q) BPSK path has no fading channel")
        fading.check()
    device = device or torch.device("cuda", torch.cuda.current_device())
    cw = None if PN_Message else np.ascontiguousarray(CodeWord_sym, np.int32)
    cw_dev = None if PN_Message else torch.from_numpy(cw).to(device)
    qam = CONSTELLATION is not None
    con = np.ascontiguousarray(CONSTELLATION, np.float32) if qam else None
    con_dev = torch.from_numpy(con).to(device) if qam else None
    frames = 0  # frames drawn at this point: numbers the random codewords
    while True:
        if PN_Message:
            cw_dev = nb.PN_CodeWords(code, pn_seed, batch, first_frame=frames, device=device)
            cw = None if device_channel else cw_dev.cpu().numpy()
        frames += batch
        if fading is not None:
            seed0, fseed0 = seed.copy(), fading.seed.copy()
            seeds_before = _SeedsAfter(seed0, code, qam)
            gain = Fading_Gains(fading.seed, fading.Lc, code.N, batch, device=device)
            words = cw_dev if PN_Message else cw_dev[None, :].expand(batch, code.N).contiguous()
            rxt = nb.AWGNChannel_Fading_GPU(seed, sigma, code, words, gain, con_dev)
        elif device_channel:
            seed0 = seed.copy()
            seeds_before = _SeedsAfter(seed0, code, qam)
            rxt = nb.AWGNChannel_GPU(seed, sigma, code, cw_dev, batch, CONSTELLATION=con_dev)
        else:
            seeds_before = []
            rx = np.empty((batch, code.N, 2) if qam else (batch, code.N * code.m), np.float32)
            for b in range(batch):
                seeds_before.append(seed.copy())
                rx[b] = nb.AWGNChannel_CPU(seed, sigma, code, cw[b] if PN_Message else cw, CONSTELLATION=con)
            rxt = torch.from_numpy(rx).to(device)
        if fading is not None:
            Lch = nb.Demodulate_QAM_Fading(code, rxt, gain, sigma, con_dev)
        else:
            Lch = nb.Demodulate(code, rxt, sigma, CONSTELLATION=con_dev)
        if decoder_method == 0:
            r = nb.Decoding_EMS(code, Lch, EMS_Nm, EMS_Nc, maxIT)
        elif decoder_method == 2:
            r = nb.Decoding_EMS(code, Lch, code.q, code.dc - 1, maxIT)  # Simulation.cpp:63-66
        else:
            r = nb.Decoding_TMM(code, Lch, maxIT, layered=(decoder_method == 3))
        errs = (r["DecodeOutput"] != (cw_dev if PN_Message else cw_dev[None, :])).sum(dim=1).cpu().numpy()
        its = r["iter_number"].cpu().numpy()
        for b in range(batch):  # account in stream order; stop where the reference's while-condition fails
            SIM.num_Frames += 1
            SIM.Total_Iteration += int(its[b])
            SIM.num_Error_Bits += int(errs[b])
            SIM.num_Error_Frames += 1 if errs[b] else 0
            done = SIM.num_Error_Frames >= leastErrorFrames and SIM.num_Frames >= leastTestFrames
            if done or (max_frames is not None and SIM.num_Frames >= max_frames):
                if b + 1 < batch:
                    seed[:] = seeds_before[b + 1]  # the reference never drew the remaining frames
                    if fading is not None:
                        fading.seed[:] = sharding.lcg_jump(fseed0, (b + 1) * sharding.fading_draws_per_frame(code.N, fading.Lc))
                return 1 if done else 0


def sweep(code, CodeWord_sym, startSNR=0.0, stopSNR=5.0, stepSNR=0.5, snrtype=0, seeds=(173, 173, 173), log=print, n_QAM=2, **kw):
    """main.cu:215-260: returns the list of NBSim, one per Eb/N0 point.  n_QAM enters sigma (main.cu:223); pass the
    constellation itself as CONSTELLATION=... for n_QAM != 2."""
    out = []
    fading_seed0 = kw["fading"].seed.tolist() if kw.get("fading") is not None else None
    s = np.float32(startSNR)
    while s <= stopSNR:
        seed = np.array(seeds, np.int32)
        SIM = NBSim(float(s))
        if kw.get("fading") is not None:  # the fading stream restarts at every point, as the noise stream does
            kw["fading"] = Fading(kw["fading"].Lc, np.array(fading_seed0, np.int32))
        Simulation_GPU(code, seed, nb.sigma_of(float(s), code.rate, snrtype, n_QAM), SIM, CodeWord_sym, **kw)
        if log:
            log(SIM.row(code.N))
        out.append(SIM)
        s = np.float32(np.float64(s) + stepSNR)
    return out
