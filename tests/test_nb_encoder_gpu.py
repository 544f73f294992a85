"""GPU tests of the GF(q) encoder (nbldpc_encode, nbldpc_encode_random), the syndrome check (nbldpc_syndrome), the per-frame
channel and statistics, and Simulation_GPU(PN_Message=1), against numpy restatements built from the CN lists, the tables of
GFInitial and the host generator."""
import os

import numpy as np
import pytest
import torch

from conftest import DATA
from test_nb_encoder_cpu import FILES, dense_h, encode_np, syndrome_np

pytestmark = pytest.mark.gpu
NB = os.path.join(DATA, "nb")


@pytest.fixture(scope="module")
def nb():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cuda_ldpc_amd import nbldpc
    return nbldpc


_cache = {}


def _code(nb, name):
    """(NBCode, TableMultiply as int64, host generator) of a shipped matrix."""
    if name not in _cache:
        q = int(open(os.path.join(NB, name)).readline().split()[2])
        mul, _, _ = nb.GFInitial(q, os.path.join(NB, "GF", "Arith.Table.GF.%d.txt" % q))
        code = nb.NBCode(os.path.join(NB, name), mul)
        _cache[name] = (code, mul.astype(np.int64), nb.generator_host(code))
    return _cache[name]


def _con(nb, q):
    return nb.Get_CONSTELLATION(os.path.join(NB, "Constellation", "GRAY_%dQAM.txt" % q), q)


def _frames_checked(B, rng, n):
    if B <= n:
        return np.arange(B)
    edge = [x for x in (0, 1, 62, 63, 64, 65, B - 2, B - 1) if x < B]
    return np.unique(np.concatenate([edge, rng.choice(B, n, replace=False)]))


@pytest.mark.parametrize("name", FILES)
def test_encoder_info_matches_host_generator(nb, name):
    code, mul, gen = _code(nb, name)
    assert code.K_info == gen["K_info"] and code.rank == gen["rank"] and code.K_info + code.rank == code.N
    assert np.array_equal(code.info_positions, gen["info_pos"])


@pytest.mark.parametrize("B", [1, 63, 64, 65, 3001])
@pytest.mark.parametrize("name", FILES)
def test_encode_matches_host_P(nb, name, B):
    code, mul, gen = _code(nb, name)
    rng = np.random.default_rng(B * 7 + len(name))
    msg = rng.integers(0, 1 << 30, (B, code.K_info), dtype=np.int32)  # only the low log2 q bits count
    cw = nb.Encode(code, torch.from_numpy(msg).cuda())
    flag = nb.Syndrome(code, cw)["flag"]
    torch.cuda.synchronize()
    cw = cw.cpu().numpy()
    assert cw.min() >= 0 and cw.max() < code.q
    assert np.array_equal(cw[:, gen["info_pos"]], msg & (code.q - 1)), "not systematic"
    sel = _frames_checked(B, rng, 8 if code.N > 1000 else 64)
    want = encode_np(gen, code.N, mul, msg[sel])
    assert np.array_equal(cw[sel], want), "differs from the host generator's encoding"
    assert not syndrome_np(code, mul, cw[sel]).any(), "H * c != 0"
    assert bool((flag == 1).all()), "the device syndrome rejects an encoded word"


@pytest.mark.parametrize("name", FILES)
def test_encode_is_linear(nb, name):
    code, mul, gen = _code(nb, name)
    rng = np.random.default_rng(5)
    B = 130
    a = rng.integers(0, code.q, (B, code.K_info), dtype=np.int32)
    b = rng.integers(0, code.q, (B, code.K_info), dtype=np.int32)
    c = 3 if code.q > 3 else 1
    ca = mul[c, a].astype(np.int32)
    ea, eb = nb.Encode(code, torch.from_numpy(a).cuda()), nb.Encode(code, torch.from_numpy(b).cuda())
    eab, eca = nb.Encode(code, torch.from_numpy(a ^ b).cuda()), nb.Encode(code, torch.from_numpy(ca).cuda())
    torch.cuda.synchronize()
    assert torch.equal(ea ^ eb, eab)
    assert np.array_equal(eca.cpu().numpy(), mul[c, ea.cpu().numpy()])


@pytest.mark.parametrize("name", FILES)
def test_encode_random_matches_rule_and_shards(nb, name):
    code, mul, gen = _code(nb, name)
    seed, B = 0xDEADBEEF12345678, 300
    cw, msg = nb.PN_CodeWords(code, seed, B, want_msg=True)
    torch.cuda.synchronize()
    assert np.array_equal(msg.cpu().numpy(), nb.pn_messages(seed, code.K_info, code.q, B)), "messages differ from the counter-based rule"
    assert torch.equal(cw, nb.Encode(code, msg)), "encode_random differs from encode of its own messages"
    tail = nb.PN_CodeWords(code, seed, B - 100, first_frame=100)
    assert torch.equal(tail, cw[100:].contiguous()), "a batch at first_frame=100 differs from frames 100.. of the longer batch"
    assert not torch.equal(nb.PN_CodeWords(code, seed + 1, B), cw)


@pytest.mark.parametrize("name", FILES)
def test_syndrome_matches_numpy(nb, name):
    code, mul, gen = _code(nb, name)
    rng = np.random.default_rng(11)
    cw = nb.PN_CodeWords(code, 3, 64).cpu().numpy()
    bad = cw.copy()
    seen = np.nonzero(dense_h(code).any(0))[0]  # symbols some check sees (the exponent-format files have all-zero columns)
    bad[np.arange(64), rng.choice(seen, 64)] ^= rng.integers(1, code.q, 64)  # one corrupted symbol each
    rnd = rng.integers(0, code.q, (64, code.N))
    high = cw + (rng.integers(0, 4, cw.shape) << 8)  # bits above log2 q are not read
    words = np.concatenate([cw, bad, rnd, high]).astype(np.int32)
    r = nb.Syndrome(code, torch.from_numpy(words).cuda())
    torch.cuda.synchronize()
    unsat = (syndrome_np(code, mul, words) != 0).sum(1)
    assert np.array_equal(r["unsat"].cpu().numpy(), unsat)
    assert np.array_equal(r["flag"].cpu().numpy(), (unsat == 0).astype(np.int32))
    assert (unsat[:64] == 0).all() and (unsat[64:192] > 0).all() and (unsat[192:] == 0).all()


def test_shipped_bds_codeword_passes_the_syndrome(nb):
    code, mul, gen = _code(nb, "BDS.576.288.GF.64.txt")
    cw = np.loadtxt(os.path.join(NB, "codeword_bds_gf64.txt"), dtype=np.int32)
    r = nb.Syndrome(code, torch.from_numpy(cw[None, :].copy()).cuda())
    assert int(r["flag"][0]) == 1 and int(r["unsat"][0]) == 0


@pytest.mark.parametrize("name", FILES)
def test_syndrome_flag_equals_decoder_ok(nb, name):
    """On DecodeOutput of noisy random codewords, a mix of frames that converge and frames that do not, flag == ok frame by frame
    for EMS and, where the code allows them, the trellis decoders (flooding and layered)."""
    code, mul, gen = _code(nb, name)
    B = 48 if code.N > 1000 else 256
    cw = nb.PN_CodeWords(code, 17, B)
    seed = np.array([173, 173, 173], np.int32)
    rx = torch.cat([nb.AWGNChannel_GPU(seed, nb.sigma_of(snr, code.rate), code, cw[i::2].contiguous(), B // 2) for i, snr in ((0, -1.0), (1, 8.0))])
    Lch = nb.Demodulate(code, rx.contiguous(), nb.sigma_of(8.0, code.rate))
    runs = [nb.Decoding_EMS(code, Lch, 2, 2, 20)]
    if name == "BDS.576.288.GF.64.txt":  # the one shipped code the trellis kernels take
        runs +=[nb.Decoding_TMM(code, Lch, 20), nb.Decoding_TMM(code, Lch, 20, layered=True)]
    for r in runs:
        s = nb.Syndrome(code, r["DecodeOutput"])
        torch.cuda.synchronize()
        assert torch.equal(s["flag"], r["ok"])
        assert 0 < int(r["ok"].sum()) < B, "the batch should hold frames that converge and frames that do not"


def _channel_cases(nb, name):
    code, mul, gen = _code(nb, name)
    cases = [None]
    if code.q in (64, 256):
        cases.append(torch.from_numpy(_con(nb, code.q)).cuda())
    return code, cases


@pytest.mark.parametrize("name", FILES)
def test_per_frame_channel_equals_single_frame_calls(nb, name):
    code, cases = _channel_cases(nb, name)
    B = 5
    cw = nb.PN_CodeWords(code, 23, B)
    for con in cases:
        qam = con is not None
        sigma = nb.sigma_of(3.0, code.rate, 0, code.q if qam else 2)
        seed = np.array([173, 171, 170], np.int32)
        rx = nb.AWGNChannel_GPU(seed, sigma, code, cw, B, CONSTELLATION=con)
        s0 = np.array([173, 171, 170], np.int32)
        for b in range(B):
            sb = nb.seed_after(s0, b, code, qam)
            one = nb.AWGNChannel_GPU(sb, sigma, code, cw[b].contiguous(), 1, CONSTELLATION=con)
            assert torch.equal(rx[b].view(torch.int32), one[0].view(torch.int32)), "frame %d (%s)" % (b, "QAM" if qam else "BPSK")
        assert np.array_equal(seed, nb.seed_after(s0, B, code, qam))
        # every frame carrying the same word: today's shared-word call
        same = cw[2:3].repeat(B, 1).contiguous()
        s1, s2 = s0.copy(), s0.copy()
        a = nb.AWGNChannel_GPU(s1, sigma, code, same, B, CONSTELLATION=con)
        b_ = nb.AWGNChannel_GPU(s2, sigma, code, cw[2].contiguous(), B, CONSTELLATION=con)
        assert torch.equal(a.view(torch.int32), b_.view(torch.int32)) and np.array_equal(s1, s2)


@pytest.mark.parametrize("name", FILES)
def test_noiseless_decode_of_random_codewords(nb, name):
    code, cases = _channel_cases(nb, name)
    B = 32 if code.N > 1000 else 128
    cw = nb.PN_CodeWords(code, 5, B)
    for con in cases:
        qam = con is not None
        sigma = nb.sigma_of(30.0 if qam else 12.0, code.rate, 0, code.q if qam else 2)
        seed = np.array([173, 173, 173], np.int32)
        rx = nb.AWGNChannel_GPU(seed, sigma, code, cw, B, CONSTELLATION=con)
        r = nb.Decoding_EMS(code, nb.Demodulate(code, rx, sigma, CONSTELLATION=con), 2, 2, 20)
        torch.cuda.synchronize()
        assert torch.equal(r["DecodeOutput"], cw) and bool((r["ok"] == 1).all())
        counters = torch.zeros(4, dtype=torch.int64, device="cuda")
        nb.Statistic(code, counters, r, cw)
        assert counters.cpu().tolist()[:2] == [0, 0] and int(counters[3]) == B


@pytest.mark.parametrize("name", ["BDS.576.288.GF.64.txt", "LDPC_N96_K48_GF256_d1_exp.txt", "LDPC_N576_K480_GF256_exp.txt"])
def test_qam_energy_of_random_codewords(nb, name):
    code, mul, gen = _code(nb, name)
    B = 8192 if code.N < 96 else 2048
    cw = nb.PN_CodeWords(code, 77, B)
    con = torch.from_numpy(_con(nb, code.q)).cuda()
    seed = np.array([173, 173, 173], np.int32)
    rx = nb.AWGNChannel_GPU(seed, 1e-6, code, cw, B, CONSTELLATION=con)
    e = float((rx.double() ** 2).sum(-1).mean())
    assert abs(e - 1.0) < 0.02, e
    zero = nb.AWGNChannel_GPU(seed, 1e-6, code, torch.zeros(code.N, dtype=torch.int32, device="cuda"), 16, CONSTELLATION=con)
    assert float((zero.double() ** 2).sum(-1).mean()) > 2.0  # the all-zero word sits on a corner point


def _recount(nb, code, seed0, sigma, batch, batches, pn_seed, device_channel, con):
    frames = errf = errb = its = 0
    seed = seed0.copy()
    con_dev = None if con is None else torch.from_numpy(con).cuda()
    for k in range(batches):
        cw = nb.PN_CodeWords(code, pn_seed, batch, first_frame=k * batch)
        if device_channel:
            rx = nb.AWGNChannel_GPU(seed, sigma, code, cw, batch, CONSTELLATION=con_dev)
        else:
            cwh = cw.cpu().numpy()
            rx = torch.from_numpy(np.stack([nb.AWGNChannel_CPU(seed, sigma, code, cwh[b], CONSTELLATION=con) for b in range(batch)])).cuda()
        r = nb.Decoding_EMS(code, nb.Demodulate(code, rx, sigma, CONSTELLATION=con_dev), 2, 2, 20)
        e = (r["DecodeOutput"] != cw).sum(1).cpu().numpy()
        frames += batch
        errf += int((e > 0).sum())
        errb += int(e.sum())
        its += int(r["iter_number"].sum())
    return frames, errf, errb, its, seed


@pytest.mark.parametrize("device_channel", [False, True])
@pytest.mark.parametrize("qam", [False, True])
def test_simulation_pn_message_counters(nb, device_channel, qam):
    from cuda_ldpc_amd.nb_simulation import NBSim, Simulation_GPU
    code, mul, gen = _code(nb, "BDS.576.288.GF.64.txt")
    con = _con(nb, 64) if qam else None
    snr = 11.5 if qam else 2.5
    sigma = nb.sigma_of(snr, code.rate, 0, 64 if qam else 2)
    batch, batches, pn_seed = 128, 3, 4242
    seed = np.array([173, 173, 173], np.int32)
    SIM = NBSim(snr)
    Simulation_GPU(code, seed, sigma, SIM, None, batch=batch, leastErrorFrames=10 ** 9, max_frames=batch * batches, device_channel=device_channel,
                   CONSTELLATION=con, PN_Message=1, pn_seed=pn_seed)
    frames, errf, errb, its, oseed = _recount(nb, code, np.array([173, 173, 173], np.int32), sigma, batch, batches, pn_seed, device_channel, con)
    assert (SIM.num_Frames, SIM.num_Error_Frames, SIM.num_Error_Bits, SIM.Total_Iteration) == (frames, errf, errb, its)
    assert np.array_equal(seed, oseed)
    assert 0 < errf < frames
