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


def _host_info_positions(code):
    """The information set of the code's generator from the host elimination alone (nbldpc_generator_host): nothing touches the device."""
    if getattr(code, "_info_pos_host", None) is None:
        code._info_pos_host = nb.generator_host(code)["info_pos"]
    return code._info_pos_host


def _check_rate_match(code, rm, short_llr, device_channel, PN_Message, CodeWord_sym, CONSTELLATION=None, fading=None):
    """Every refusal of a rate-matched point, before anything touches the device."""
    if CONSTELLATION is not None or fading is not None:
        raise ValueError("rate_match runs over BPSK: the simulations have no rate-matched QAM or fading chain (DESIGN.md 4.19)")
    if not device_channel:
        raise ValueError("rate_match needs device_channel=True: select, the channel at N := E and the fused receive run on the device")
    if rm.N != code.N:
        raise ValueError("rate_match is over N=%d symbols, the code has N=%d" % (rm.N, code.N))
    if not (np.isfinite(short_llr) and short_llr > 0):
        raise ValueError("short_llr must be finite and > 0, not %r" % (short_llr,))
    if rm.n_short:
        if not np.isin(rm.shorten, _host_info_positions(code)).all():
            raise ValueError("rate_match shortens a parity position of the code's generator; only information positions can be agreed to be 0")
        if not PN_Message and np.any(np.asarray(CodeWord_sym).reshape(-1)[rm.shorten] != 0):
            raise ValueError("CodeWord_sym is not 0 at every shortened position")


# The BPSK receive side of a rate-matched batch: the fused call or its composition Demodulate_NQ -> RM_Recover / RM_Combine, whichever
# profiles/nb_rm_time.txt measured faster.  The fused call won every measured BPSK case (0.46 .. 0.97 of its
# composition) but one: the combine at q = 256 on a one-lap profile with a mask in which no frame is done, 1.03 (with half of the frames
# done: 0.63).  n_done: how many frames of the mask are done (None: no mask).  Both give the same bits (tests/test_nb_rm_gpu.py).
def _fused_is_faster(rm, q, combine, n_done):
    return not (combine and q >= 256 and rm.laps == 1 and not n_done)


def _rm_receive(rm, q, rx, sigma, short_llr, acc=None, done=None, n_done=None, fused=None):
    if _fused_is_faster(rm, q, acc is not None, n_done) if fused is None else fused:
        if acc is None:
            return nb.RM_Demodulate_Recover(rm, q, rx, sigma, short_llr)
        return nb.RM_Demodulate_Combine(rm, q, rx, sigma, acc, done, short_llr)
    Lrx = nb.Demodulate_NQ(rm.E, q, rx, sigma)
    return nb.RM_Recover(rm, q, Lrx, short_llr) if acc is None else nb.RM_Combine(rm, q, Lrx, acc, done, short_llr)


def _decode(code, Lch, decoder_method, EMS_Nm, EMS_Nc, maxIT, qspa_tier="lds"):
    if decoder_method == 0:
        return nb.Decoding_EMS(code, Lch, EMS_Nm, EMS_Nc, maxIT)
    if decoder_method == 2:
        return nb.Decoding_EMS(code, Lch, code.q, code.dc - 1, maxIT)  # Simulation.cpp:63-66
    if decoder_method in (4, 5):
        return nb.Decoding_QSPA(code, Lch, maxIT, layered=(decoder_method == 5), tier=qspa_tier)  # ours: the reference stops at 3
    return nb.Decoding_TMM(code, Lch, maxIT, layered=(decoder_method == 3))


def _simulation_rm(code, seed, sigma, SIM, CodeWord_sym, rm, short_llr, EMS_Nm, EMS_Nc, maxIT, batch, leastErrorFrames, leastTestFrames,
                   max_frames, device, decoder_method, PN_Message, pn_seed, qspa_tier="lds"):
    """Simulation_GPU with rate_match=rm, over BPSK: select -> the per-frame channel at N := E -> the fused receive -> the decoder.
    The seed roll-back is by E."""
    words = None if PN_Message else torch.from_numpy(np.ascontiguousarray(CodeWord_sym, np.int32)).to(device)[None, :].expand(batch, code.N).contiguous()
    frames = 0
    while True:
        if PN_Message:
            words = nb.PN_CodeWords(code, pn_seed, batch, first_frame=frames, device=device, rate_match=rm)
        frames += batch
        tx = nb.RM_Select(rm, words)
        seed0 = seed.copy()
        rx = nb.AWGNChannel_RM_GPU(seed, sigma, rm, code.q, tx)
        Lch = _rm_receive(rm, code.q, rx, sigma, short_llr)
        r = _decode(code, Lch, decoder_method, EMS_Nm, EMS_Nc, maxIT, qspa_tier)
        errs = (r["DecodeOutput"] != words).sum(dim=1).cpu().numpy()
        its = r["iter_number"].cpu().numpy()
        for b in range(batch):  # account in stream order; stop where the reference's while-condition fails
            SIM.num_Frames += 1
            SIM.Total_Iteration += int(its[b])
            SIM.num_Error_Bits += int(errs[b])
            SIM.num_Error_Frames += 1 if errs[b] else 0
            done = SIM.num_Error_Frames >= leastErrorFrames and SIM.num_Frames >= leastTestFrames
            if done or (max_frames is not None and SIM.num_Frames >= max_frames):
                if b + 1 < batch:
                    seed[:] = nb.seed_after(seed0, b + 1, code, E=rm.E)  # the remaining frames were never drawn
                return 1 if done else 0


def Simulation_GPU(code, seed, sigma, SIM, CodeWord_sym, EMS_Nm=2, EMS_Nc=2, maxIT=20, batch=1024, leastErrorFrames=50,
                   leastTestFrames=1000, max_frames=None, device=None, device_channel=False, decoder_method=0, CONSTELLATION=None,
                   PN_Message=0, pn_seed=0, fading=None, rate_match=None, short_llr=1.0e4, qspa_tier="lds"):
    """One Eb/N0 point. `seed` (int32[3]) advances exactly as far as the reference would have drawn.
    device_channel: generate the noise on the GPU (same uniforms, device libm) instead of the host, frame by frame.
    decoder_method (define.h:37, Simulation.cpp:54-70): 0 EMS, 1 trellis min-max, 2 log-QSPA = EMS(q, dc-1), 3 layered TMM;
    4 and 5 are ours, the reference stops at 3: the FHT sum-product decoder (Decoding_QSPA; include/nbldpc.h, "FHT sum-product"),
    flooding and layered (layered=True; "FHT sum-product, layered schedule").  qspa_tier ("lds", "workspace" or "auto"): the tier of
    Decoding_QSPA those two run on; "auto" takes the workspace tier for the codes the LDS tier refuses.
    CONSTELLATION (host float32 [q, 2], Get_CONSTELLATION): the n_QAM = q branches of Modulate / AWGNChannel_CPU / Demodulate
    (one constellation point per code symbol) instead of BPSK; the caller passes the sigma of that n_QAM.
    PN_Message=1: every frame sends its own random codeword in place of CodeWord_sym (may be None): frame i of the point is
    PN_CodeWords(code, pn_seed, ..., first_frame=i) (nbldpc_encode_random), and its errors are counted against that word.  The
    decoders stop on their own syndrome, so the stop rule and the seed roll-back are unchanged.
    fading (a Fading): flat Rayleigh block fading with receiver CSI over the QAM channel (include/nbldpc.h): every batch draws one gain
    per block of Lc symbols and frame from the fading stream, fading.seed (ceil(N / Lc) draws per frame; rolled back with the noise seed
    to the frame at which the reference would have stopped), sends the points through nbldpc_fading_channel_device_qam_frames -- one
    word for all frames is expanded to [batch, N] first, the draws are where the per-frame channel puts them -- and demodulates against
    the faded points (Demodulate_QAM_Fading).  Needs CONSTELLATION and device_channel=True.
    rate_match (a RateMatch over code.N symbols; include/nbldpc.h, "rate matching"): every frame sends the profile's E symbols only --
    RM_Select -> the per-frame channel at N := E (4 E m draws per frame) -> the fused receive -> the decoder, any decoder_method -- with
    -short_llr on the shortened symbols and 0 on the punctured ones.  The seed roll-back is by E; the stop rule is unchanged.  Needs
    device_channel=True and runs over BPSK: CONSTELLATION and fading are refused with it.  Refused before the
    device is touched: a shortened position outside the information set of the code's generator, and PN_Message=0 with a CodeWord_sym
    that is not 0 at every shortened position (PN_Message=1 forces the message symbols there to 0: PN_CodeWords(rate_match=...)).  The
    caller passes the sigma of the derived rate (K' - n_short) / E; sweep does."""
    if PN_Message not in (0, 1):
        raise ValueError("PN_Message must be 0 (CodeWord_sym for every frame) or 1 (random codewords)")
    if rate_match is not None:
        _check_rate_match(code, rate_match, short_llr, device_channel, PN_Message, CodeWord_sym, CONSTELLATION, fading)
    if fading is not None:  # every refusal before anything touches the device
        if not isinstance(fading, Fading):
            raise ValueError("fading must be a Fading (block length and the seed of the fading stream), not %r" % (fading,))
        if not device_channel:
            raise ValueError("fading needs device_channel=True: the gains and the channel that applies them run on the device")
        if CONSTELLATION is None:
            raise ValueError("fading needs CONSTELLATION: the GF(q) BPSK path has no fading channel")
        fading.check()
    device = device or torch.device("cuda", torch.cuda.current_device())
    if rate_match is not None:
        return _simulation_rm(code, seed, sigma, SIM, CodeWord_sym, rate_match, short_llr, EMS_Nm, EMS_Nc, maxIT, batch, leastErrorFrames,
                              leastTestFrames, max_frames, device, decoder_method, PN_Message, pn_seed, qspa_tier)
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
        r = _decode(code, Lch, decoder_method, EMS_Nm, EMS_Nc, maxIT, qspa_tier)
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


def sweep(code, CodeWord_sym, startSNR=0.0, stopSNR=5.0, stepSNR=0.5, snrtype=0, seeds=(173, 173, 173), log=print, n_QAM=2, qspa_tier="lds",
          **kw):
    """main.cu:215-260: returns the list of NBSim, one per Eb/N0 point.  n_QAM enters sigma (main.cu:223); pass the
    constellation itself as CONSTELLATION=... for n_QAM != 2.  With rate_match=rm the rate in sigma is the derived code's,
    (K' - n_short) / E.  qspa_tier: as in Simulation_GPU."""
    out = []
    fading_seed0 = kw["fading"].seed.tolist() if kw.get("fading") is not None else None
    rm = kw.get("rate_match")
    rate = code.rate if rm is None else np.float32(len(_host_info_positions(code)) - rm.n_short) / np.float32(rm.E)
    s = np.float32(startSNR)
    while s <= stopSNR:
        seed = np.array(seeds, np.int32)
        SIM = NBSim(float(s))
        if kw.get("fading") is not None:  # the fading stream restarts at every point, as the noise stream does
            kw["fading"] = Fading(kw["fading"].Lc, np.array(fading_seed0, np.int32))
        Simulation_GPU(code, seed, nb.sigma_of(float(s), rate, snrtype, n_QAM), SIM, CodeWord_sym, qspa_tier=qspa_tier, **kw)
        if log:
            log(SIM.row(code.N))
        out.append(SIM)
        s = np.float32(np.float64(s) + stepSNR)
    return out


def Simulation_HARQ_GPU(code, seed, sigma, SIM, rvs, CodeWord_sym=None, EMS_Nm=2, EMS_Nc=2, maxIT=20, batch=1024, leastErrorFrames=50,
                        leastTestFrames=1000, max_batches=None, device=None, decoder_method=0, PN_Message=1, pn_seed=0,
                        short_llr=1.0e4, compact=True, log=print, keep=None, qspa_tier="lds"):
    """One Eb/N0 point of HARQ with symbol-LLR combining on the device channel, over BPSK.  rvs = [rm_0, ..., rm_{T-1}]: the profile of each
    transmission (RateMatch.circular or RateMatch over code.N symbols, all with the same shortened positions).  SIM is the binary
    side's HarqCounters, counted in symbols: bits_sent is the sum of E_t * m over the transmissions each frame used.

    A batch: rvs[0] is sent for all B frames (RM_Select -> the per-frame channel at N := E_0 -> the fused receive, recover semantics)
    and decoded; the decoder's own ok (its syndrome) is the ACK, so no Syndrome call is needed, and `undetected` counts acknowledged
    frames whose decoded word is not the word sent.  For t = 1 .. T-1, while a frame is unacknowledged: rvs[t] is drawn for all frames
    and combined into L_acc under done = ok, and the unacknowledged frames alone are decoded -- index_select on the frame-outer L_acc,
    index_copy_ of the results -- unless compact=False, which decodes the whole batch again.  Both give the same counters because a
    frame's decode result (DecodeOutput, iter_number, ok) does not depend on its batch mates: every decoder kernel works one frame
    at a time from that frame's L_ch alone (tests/test_nb_rm_gpu.py holds the decoders to that).

    Draws: transmission t of a batch owns 4 * E_t * m * B draws of the noise stream, used or not -- `seed` (int32[3])
    is advanced by the sum over all T transmissions after every batch, whatever was acknowledged.
    PN_Message=1 (default): frame i sends PN_CodeWords(code, pn_seed, first_frame=i, rate_match=rvs[0]); PN_Message=0: CodeWord_sym
    for every frame (0 at the shortened positions).  The stop rule is the binary one: never_acked + undetected >= leastErrorFrames and
    num_Frames >= leastTestFrames, tested after every batch.  keep (a list) receives (DecodeOutput, ok, words) of every batch.
    qspa_tier: as in Simulation_GPU."""
    from .simulation import format_harq_row
    if PN_Message not in (0, 1):
        raise ValueError("PN_Message must be 0 (CodeWord_sym for every frame) or 1 (random codewords)")
    if not PN_Message and CodeWord_sym is None:
        raise ValueError("PN_Message=0 needs CodeWord_sym")
    rvs = list(rvs) if rvs is not None else []
    if not rvs:
        raise ValueError("rvs must hold at least one profile")
    for t, rm in enumerate(rvs):
        _check_rate_match(code, rm, short_llr, True, PN_Message, CodeWord_sym)
        if not np.array_equal(rm.shorten, rvs[0].shorten):
            raise ValueError("rvs[%d] shortens other positions than rvs[0]: the shortened symbols are fixed by the codeword, not by the transmission" % t)
    T = len(rvs)
    if not SIM.acked:
        SIM.acked, SIM.undetected = [0] * T, [0] * T
    if len(SIM.acked) != T:
        raise ValueError("SIM holds counters of %d transmissions, rvs has %d" % (len(SIM.acked), T))
    device = device or torch.device("cuda", torch.cuda.current_device())
    B, q, m = batch, code.q, code.m
    info_bits = (len(_host_info_positions(code)) - rvs[0].n_short) * m
    words = None if PN_Message else torch.from_numpy(np.ascontiguousarray(CodeWord_sym, np.int32)).to(device)[None, :].expand(B, code.N).contiguous()
    cnt = torch.zeros(2 * T + 3, dtype=torch.int64, device=device)  # acked[T], undetected[T], never, bits, iterations
    batches = 0
    while True:
        SIM.num_Frames += B
        cnt.zero_()
        if PN_Message:
            words = nb.PN_CodeWords(code, pn_seed, B, first_frame=batches * B, device=device, rate_match=rvs[0])
        acked = torch.zeros(B, dtype=torch.bool, device=device)
        for t, rm in enumerate(rvs):
            my_seed = seed.copy()
            seed[:] = nb.seed_after(seed, B, code, E=rm.E)  # owned by this transmission whether it is used or not
            n_done = int(acked.sum()) if t else 0
            if n_done == B:
                continue
            active = ~acked
            rx = nb.AWGNChannel_RM_GPU(my_seed, sigma, rm, q, nb.RM_Select(rm, words))
            if t == 0:
                acc = _rm_receive(rm, q, rx, sigma, short_llr)
                r = _decode(code, acc, decoder_method, EMS_Nm, EMS_Nc, maxIT, qspa_tier)
                out, iters, ok = r["DecodeOutput"], r["iter_number"], r["ok"]
            else:
                _rm_receive(rm, q, rx, sigma, short_llr, acc=acc, done=ok, n_done=n_done)
                if compact:
                    idx = torch.nonzero(active).view(-1)
                    r = _decode(code, acc.index_select(0, idx), decoder_method, EMS_Nm, EMS_Nc, maxIT, qspa_tier)
                    out.index_copy_(0, idx, r["DecodeOutput"])
                    iters.index_copy_(0, idx, r["iter_number"])
                    ok.index_copy_(0, idx, r["ok"])
                else:  # an acknowledged frame's L_acc has not changed: it decodes to what it decoded to
                    r = _decode(code, acc, decoder_method, EMS_Nm, EMS_Nc, maxIT, qspa_tier)
                    out, iters, ok = r["DecodeOutput"], r["iter_number"], r["ok"]
            now = (ok != 0) & active
            wrong = (out != words).any(1)
            cnt[t] += now.sum()
            cnt[T + t] += (now & wrong).sum()
            cnt[2 * T + 1] += rm.E * m * active.sum()
            cnt[2 * T + 2] += iters[active].sum()
            acked |= now
        cnt[2 * T] += (~acked).sum()
        if keep is not None:
            keep.append((out, ok, words))
        c = cnt.cpu().tolist()
        for t in range(T):
            SIM.acked[t] += c[t]
            SIM.undetected[t] += c[T + t]
        SIM.never_acked += c[2 * T]
        SIM.bits_sent += c[2 * T + 1]
        SIM.Total_Iteration += c[2 * T + 2]
        batches += 1
        errors = SIM.never_acked + sum(SIM.undetected)
        stop = errors >= leastErrorFrames and SIM.num_Frames >= leastTestFrames
        last = max_batches is not None and batches >= max_batches
        if log and (stop or last):
            log(format_harq_row(SIM, info_bits))
        if stop or last:
            return 1 if stop else 0


def sweep_harq(code, rvs, CodeWord_sym=None, startSNR=0.0, stopSNR=5.0, stepSNR=0.5, snrtype=0, seeds=(173, 173, 173), log=print,
               qspa_tier="lds", **kw):
    """The sweep of `sweep` over Simulation_HARQ_GPU: a list of HarqCounters, one per Eb/N0 point.  sigma comes from nbldpc.sigma_of
    (BPSK) with the rate of the FIRST transmission, (K' - n_short) / E_0: the operating point is named by what is sent when nothing goes
    wrong, and the later transmissions run over the same channel."""
    from .simulation import HarqCounters
    out = []
    rate = np.float32(len(_host_info_positions(code)) - rvs[0].n_short) / np.float32(rvs[0].E)
    s = np.float32(startSNR)
    while s <= stopSNR:
        seed = np.array(seeds, np.int32)
        SIM = HarqCounters()
        SIM.SNR = float(s)
        Simulation_HARQ_GPU(code, seed, nb.sigma_of(float(s), rate, snrtype), SIM, rvs, CodeWord_sym, log=log, qspa_tier=qspa_tier, **kw)
        out.append(SIM)
        s = np.float32(np.float64(s) + stepSNR)
    return out
