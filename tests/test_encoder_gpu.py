"""GPU tests of the systematic encoder (bldpc_encode, bldpc_encode_random), the syndrome check (bldpc_syndrome) and
Simulation_GPU(PN_Message=1), against numpy restatements built from the block shifts and the host generator."""
import os

import numpy as np
import pytest
import torch

from conftest import DATA
from test_encoder_cpu import encode_np, syndrome_np

pytestmark = pytest.mark.gpu

BL = os.path.join(DATA, "bldpc")

CODES = {  # name: (file, J, L, Z)
    "J4_L24_Z96": ("J4_L24_Z96_BlockH.txt", 4, 24, 96),
    "J32_L64_Z64": ("J32_L64_Z64_BlockH.txt", 32, 64, 64),
    "J24_L60_Z160": ("J24_L60_Z160_BlockH.txt", 24, 60, 160),  # singular parity part
    "J48_L60_Z160": ("J48_L60_Z160_BlockH.txt", 48, 60, 160),  # rank-deficient
    "PON": ("PON_LDPC.txt", 12, 69, 256),
    "J15_L30_Z1280": ("J15_L30_Z1280_BlockH.txt", 15, 30, 1280),
}


@pytest.fixture(scope="module")
def C():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_ldpc_amd
    return cuda_ldpc_amd


_cache = {}


def _code(C, name):
    if name not in _cache:
        f, J, L, Z = CODES[name]
        H, _, _ = C.Get_H(os.path.join(BL, f), J, L)
        code = C.BinaryCode.from_shifts(H, J, L, Z)
        _cache[name] = (code, H, C.generator_host(H, J, L, Z))
    return _cache[name]


def _frames_checked(F, rng, n=48):
    """All frames of a small batch; of a large one the edges of the 64-frame groups and a random sample."""
    if F <= 128:
        return np.arange(F)
    edge = [0, 1, 62, 63, 64, 65, F - 4, F - 3, F - 2, F - 1]
    return np.unique(np.concatenate([edge, rng.choice(F, n, replace=False)]))


@pytest.mark.parametrize("name", list(CODES))
def test_encoder_info_matches_host_generator(C, name):
    code, H, gen = _code(C, name)
    assert code.K_info == gen["K_info"] and code.rank == gen["rank"]
    assert np.array_equal(code.info_positions, gen["info_pos"])


@pytest.mark.parametrize("F", [1, 63, 64, 65, 4099])
@pytest.mark.parametrize("name", list(CODES))
def test_encode_matches_host_P(C, name, F):
    code, H, gen = _code(C, name)
    J, L, Z = CODES[name][1:]
    rng = np.random.default_rng(F * 31 + len(name))
    msg = rng.integers(0, 1 << 31, (code.K_info, F), dtype=np.int32)  # only bit 0 counts
    cw = C.Encode(code, torch.from_numpy(msg).cuda())
    torch.cuda.synchronize()
    cw = cw.cpu().numpy()
    assert set(np.unique(cw)) <= {0, 1}
    assert np.array_equal(cw[gen["info_pos"]], msg & 1), "not systematic"
    sel = _frames_checked(F, rng)
    assert np.array_equal(cw[:, sel], encode_np(gen, code.N, msg[:, sel])), "differs from the host generator's encoding"
    cols = np.arange(F) if F <= 1024 else np.unique(np.concatenate([sel, rng.choice(F, 512, replace=False)]))
    assert not syndrome_np(H, J, L, Z, cw[:, cols].astype(np.uint8)).any(), "H * c != 0"


@pytest.mark.parametrize("name", list(CODES))
def test_encode_is_linear(C, name):
    code, H, gen = _code(C, name)
    rng = np.random.default_rng(5)
    F = 130
    a = torch.from_numpy(rng.integers(0, 2, (code.K_info, F), dtype=np.int32)).cuda()
    b = torch.from_numpy(rng.integers(0, 2, (code.K_info, F), dtype=np.int32)).cuda()
    ea, eb, eab = C.Encode(code, a), C.Encode(code, b), C.Encode(code, a ^ b)
    assert torch.equal(ea ^ eb, eab)


@pytest.mark.parametrize("name", list(CODES))
def test_encode_random_matches_rule_and_shards(C, name):
    from cuda_ldpc_amd.bldpc import pn_messages
    code, H, gen = _code(C, name)
    seed, F = 0xDEADBEEF12345678, 200 if code.K_info > 8000 else 300
    cw, msg = C.PN_CodeWords(code, seed, F, first_frame=0, want_msg=True)
    torch.cuda.synchronize()
    want = pn_messages(seed, code.K_info, F)
    assert np.array_equal(msg.cpu().numpy(), want), "messages differ from the counter-based rule"
    assert torch.equal(cw, C.Encode(code, msg)), "encode_random differs from encode of its own messages"
    tail = C.PN_CodeWords(code, seed, F - 100, first_frame=100)
    assert torch.equal(tail, cw[:, 100:].contiguous()), "a batch at first_frame=100 differs from frames 100.. of the longer batch"
    other = C.PN_CodeWords(code, seed + 1, F)
    assert not torch.equal(other, cw)


@pytest.mark.parametrize("name", list(CODES))
def test_syndrome_matches_numpy(C, name):
    code, H, gen = _code(C, name)
    J, L, Z = CODES[name][1:]
    rng = np.random.default_rng(11)
    F = 333
    D = rng.integers(0, 2, (code.N + 1, F), dtype=np.int32)
    cw = C.PN_CodeWords(code, 3, 64).cpu().numpy()
    D[:code.N, :64] = cw  # valid codewords
    D[:code.N, 64:128] = cw
    D[rng.integers(0, code.N, 64), np.arange(64, 128)] ^= 1  # one flipped bit each
    want = syndrome_np(H, J, L, Z, D[:code.N].astype(np.uint8)).sum(0).astype(np.int32)
    Dt = torch.from_numpy(D).cuda()
    r = C.Syndrome(code, Dt, into_flag_row=True)
    torch.cuda.synchronize()
    assert np.array_equal(r["unsat"].cpu().numpy(), want)
    assert np.array_equal(Dt[code.N].cpu().numpy(), (want == 0).astype(np.int32))
    assert np.array_equal(Dt[:code.N].cpu().numpy(), D[:code.N]), "rows 0..N-1 of D changed"
    assert (want[:64] == 0).all() and (want[64:128] > 0).all()
    r2 = C.Syndrome(code, Dt[:code.N].contiguous(), into_flag_row=False)
    assert np.array_equal(r2["flag"].cpu().numpy(), (want == 0).astype(np.int32))


def test_table_code_is_unsupported(C):
    from cuda_ldpc_amd._lib import LdpcError
    f, J, L, Z = CODES["J4_L24_Z96"]
    H, wc, wv = C.Get_H(os.path.join(BL, f), J, L)
    code = C.BinaryCode.from_table(J, L, Z, wc, wv, C.Transform_H(H, J, L, Z, wc, wv))
    with pytest.raises(LdpcError, match=r"\(-5\)"):
        code.K_info
    with pytest.raises(LdpcError, match=r"\(-5\)"):
        C.PN_CodeWords(code, 1, 64)
    with pytest.raises(LdpcError, match=r"\(-5\)"):
        C.Syndrome(code, torch.zeros((code.N + 1, 64), dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("name", ["J4_L24_Z96", "PON", "J24_L60_Z160"])
def test_decoder_symmetry_on_codewords(C, name):
    """Min-sum commutes with flipping the channel signs of a codeword: decoding y0 * (1 - 2c) gives D0 ^ c, except on
    frames where an a-posteriori value is an exact +-0 (its hard decision does not flip)."""
    code, H, gen = _code(C, name)
    F = 256
    seed = np.array([173, 173, 173], np.int32)
    y0 = C.AWGNChannel_CPU(seed, C.sigma_of(2.0 if name != "J4_L24_Z96" else 1.5), code.N, F)
    c = C.PN_CodeWords(code, 99, F)
    y0t = torch.from_numpy(y0).cuda()
    y = (y0t * (1 - 2 * c).to(torch.float32)).contiguous()
    r0 = C.LDPC_Decoder_GPU(code, y0t, max_iter=20, exit_mode=C.EXIT_FIXED, want_app=True)
    r1 = C.LDPC_Decoder_GPU(code, y, max_iter=20, exit_mode=C.EXIT_FIXED, want_app=True)
    torch.cuda.synchronize()
    keep = ~(r0["app"] == 0).any(0)
    assert keep.sum() > F // 2
    want = r0["D"][:code.N] ^ c
    assert torch.equal(r1["D"][:code.N][:, keep], want[:, keep])
    assert torch.equal(r1["app"][:, keep], (r0["app"] * (1 - 2 * c).to(torch.float32))[:, keep])


def _recount(C, code, H, snr, F, batches, pn_seed, maxIT):
    """The counters of Simulation_GPU(PN_Message=1) recomputed in numpy from the same codewords, channel and decodes."""
    J, L, Z = code.J, code.L, code.Z
    seed = np.array([173, 173, 173], np.int32)
    sigma = C.sigma_of(snr, 1, code.K / code.N)
    tot = np.zeros(5, np.int64)
    zero_flags = 0
    for b in range(batches):
        cw = C.PN_CodeWords(code, pn_seed, F, first_frame=b * F)
        y = C.AWGNChannel_CPU(seed, sigma, code.N, F, CodeWord=cw.cpu().numpy())
        r = C.LDPC_Decoder_GPU(code, torch.from_numpy(y).cuda(), max_iter=maxIT, exit_mode=C.EXIT_FIXED)
        D = r["D"].cpu().numpy()
        zero_flags += int(D[code.N].sum())
        cwn = cw.cpu().numpy()
        errs = (D[:code.K] != cwn[:code.K]).sum(0)
        ok = ~syndrome_np(H, J, L, Z, D[:code.N].astype(np.uint8)).any(0)
        tot += [np.sum((errs != 0) | ~ok), errs.sum(), maxIT * F, np.sum((errs != 0) & ok), np.sum((errs == 0) & ~ok)]
    return tot, zero_flags


@pytest.mark.parametrize("snr,device_channel", [(1.6, False), (1.6, True), (8.0, False)])
def test_simulation_pn_message_counters(C, snr, device_channel):
    from cuda_ldpc_amd.simulation import Simulation_GPU
    code, H, gen = _code(C, "J4_L24_Z96")
    F, batches, maxIT, pn_seed = 512, 3, 20, 4242
    SIM = C.SimCounters()
    Simulation_GPU(code, np.array([173, 173, 173], np.int32), C.sigma_of(snr, 1, code.K / code.N), SIM, Num_Frames_OneTime=F,
                   maxIT=maxIT, exit_mode=C.EXIT_FIXED, max_batches=batches, log=None, device_channel=device_channel,
                   PN_Message=1, pn_seed=pn_seed)
    got = [SIM.num_Error_Frames, SIM.num_Error_Bits, SIM.Total_Iteration, SIM.num_False_Frames, SIM.num_Alarm_Frames]
    assert SIM.num_Frames == F * batches
    if device_channel:  # device libm: samples may differ from the host channel in the last ulp; same statistics
        assert got[2] == maxIT * F * batches and 0 < got[0] < F * batches
        return
    want, zero_flags = _recount(C, code, H, snr, F, batches, pn_seed, maxIT)
    assert got == want.tolist()
    if snr >= 8:
        assert got[0] == 0 and got[1] == 0
        assert zero_flags == 0, "the zero-word flag would have counted every frame as an error frame"
    else:
        assert got[0] > 0
