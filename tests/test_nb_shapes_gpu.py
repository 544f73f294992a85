"""The GF(q) decoder kernels on the random codes of tests/nb_shape_cases.py -- the shapes the reference's matrices and the (2, 4)
synthetics of test_nbldpc_gpu.py skip: k_nb_ems<Q, 8> (column weights 3 and 4), its tail loop past 96 columns, rows of weight 2,
k_nb_ems_wide<128> and the wide kernel with idle groups / dv 3 / irregular rows, k_nb_ems_hbm at GF(4) / GF(8), on explicit-stack
rows of weight 7 ... 12, with both walks in one launch and with several chunk passes, k_nb_tmm on rows of 7 and 8 edges, dv 3 and 4
and 63 levels.  Every frame of every batch against the CPU oracle: symbols, iteration counts, flags and the bits of the final LLR
and L_c2v.  All comparisons are exact.  tests/test_nb_shapes_cpu.py vouches for the files, the routing and the inputs."""
import numpy as np
import pytest
import torch

import nb_shape_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nb():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cuda_ldpc_amd import nbldpc
    return nbldpc


_CODES = {}


def make_code(nb, case):
    mpath, gpath = S.files(case)
    mul, _, _ = nb.GFInitial(case.q, gpath)
    return nb.NBCode(mpath, mul)


def code_of(nb, case):
    if case.id not in _CODES:
        _CODES[case.id] = make_code(nb, case)
    return _CODES[case.id]


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def assert_frames(r, want, frames, what, state=True):
    """r: a decode call's dict (device); want[i]: the oracle's dict for frame frames[i] of the call."""
    out, it, ok = r["DecodeOutput"].cpu().numpy(), r["iter_number"].cpu().numpy(), r["ok"].cpu().numpy()
    LLR = r["LLR"].cpu().numpy() if state else None
    c2v = r["L_c2v"].cpu().numpy() if state else None
    for w, b in zip(want, frames):
        tag = "%s, frame %d" % (what, b)
        assert (int(it[b]), int(ok[b])) == (w["it"], w["ok"]), tag + ": (iterations, ok)"
        assert np.array_equal(out[b], w["out"]), tag + ": symbols"
        if state:
            assert np.array_equal(bits(LLR[b]), bits(w["LLR"])), tag + ": LLR bits"
            assert np.array_equal(bits(c2v[b]), bits(w["c2v"])), tag + ": L_c2v bits"


def assert_same_call(a, b, what, state=True):
    for k in ("DecodeOutput", "iter_number", "ok"):
        assert torch.equal(a[k], b[k]), what + ": " + k
    for k in (("LLR", "L_c2v") if state else ()):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), what + ": " + k


@pytest.mark.parametrize("cid", S.IDS)
def test_ems_equals_the_oracle(nb, orc, cid):
    case = S.BY_ID[cid]
    code = code_of(nb, case)
    Lch = S.inputs(orc, case)
    want = S.want_ems(orc, case)
    ok, what = S.spread_ok(case, want)  # this machine's numpy may have drawn another graph than the one the Eb/N0 were chosen on
    assert ok, "EMS " + what
    Lt = torch.from_numpy(Lch.copy()).cuda()
    r = nb.Decoding_EMS(code, Lt, 2, 2, S.MAX_ITER, want_state=True)
    assert code.last_kernel == case.kernel
    torch.cuda.synchronize()
    assert_frames(r, want, range(Lch.shape[0]), "EMS(2, 2) " + cid)
    if cid == "tail_q64":  # the pipeline is not offered ((16 - 4) * 8 < 100 columns): the production call stays on k_nb_ems
        p = nb.Decoding_EMS(code, Lt, 2, 2, S.MAX_ITER)
        assert code.last_kernel == "k_nb_ems" and p["LLR"] is None and p["L_c2v"] is None
        torch.cuda.synchronize()
        assert_same_call(r, p, "call without state outputs", state=False)


NC_RULE = [c.id for c in S.CASES if c.drop and c.dc <= 8]


@pytest.mark.parametrize("cid", NC_RULE)
def test_per_row_nc_rule_on_irregular_rows(nb, orc, cid):
    """EMS_NC == maxdc - 1 means `every configuration of every row`: Nc = w - 1 per row (LDPC_Decoder.cpp:294-297), on rows of two
    weights in one launch.  With maxdc = dc the rule only bounds the walk where it ends anyway; with maxdc = dc - 1 (the dc = 8
    codes) it decides: EMS_NC = 6 == maxdc - 1 lets the rows of weight 8 deviate in all 7 positions, which Nc = 6 would forbid."""
    case = S.BY_ID[cid]
    assert NC_RULE == ["dv3_q16", "dv3_q64", "dv4_q32", "tail_q16", "tail_q64", "wide128", "wide128_dv3", "hbm_q4", "hbm_q8", "dc8_q16",
                       "dc8_q32_dv3", "big_q16"]
    code = code_of(nb, case)
    Lch = S.inputs(orc, case)
    Lt = torch.from_numpy(Lch.copy()).cuda()
    forms = [(3, case.dc - 1, 0, None)]
    if case.dc == 8:
        forms += [(2, 7, 8, 8),   # maxdc given: the rule fires, rows of weight 7 walk with Nc = 6
                  (2, 6, 8, 8),   # one below: the rule does not fire, Nc = 6 on every row
                  (2, 6, 7, 7)]   # the rule fires on EMS_NC = 6: Nc = 7 on the rows of weight 8, 6 on those of weight 7
    for Nm, Nc, maxdc, dcmax_cfg in forms:
        want = S.want_ems(orc, case, Nm, Nc, dcmax_cfg)
        r = nb.Decoding_EMS(code, Lt, Nm, Nc, S.MAX_ITER, maxdc=maxdc, want_state=True)
        assert code.last_kernel == case.kernel
        torch.cuda.synchronize()
        assert_frames(r, want, range(Lch.shape[0]), "EMS(%d, %d, maxdc %d) %s" % (Nm, Nc, maxdc, cid))


@pytest.mark.parametrize("cid", S.IDS)
def test_trellis_decoders_equal_the_oracle_or_refuse(nb, orc, cid):
    from cuda_ldpc_amd._lib import LdpcError
    case = S.BY_ID[cid]
    code = code_of(nb, case)
    Lch = S.inputs(orc, case)
    Lt = torch.from_numpy(Lch.copy()).cuda()
    if not case.tmm:
        assert cid.startswith("wide") or cid in ("hbm_q4", "hbm_q8", "dc12_q64", "hbm256_mixed", "big_q16", "ladder64")
        before = code.last_kernel
        for layered in (False, True):
            with pytest.raises(LdpcError, match=r"\(-5\): .*\S"):
                nb.Decoding_TMM(code, Lt, S.MAX_ITER, layered=layered, want_state=True)
        assert code.last_kernel == before, "a refused call launches nothing"
        return
    for layered in (False, True):
        want = S.want_tmm(orc, case, layered)
        ok, what = S.spread_ok(case, want)
        assert ok, ("layered " if layered else "flooding ") + "trellis " + what
        r = nb.Decoding_TMM(code, Lt, S.MAX_ITER, layered=layered, want_state=True)
        assert code.last_kernel == ("k_nb_tmm (layered)" if layered else "k_nb_tmm")
        torch.cuda.synchronize()
        assert_frames(r, want, range(Lch.shape[0]), ("layered " if layered else "flooding ") + "trellis " + cid)


def noisy_batch(nb, code, B, snr):
    """B frames of the all-zero codeword from the device channel (the reference's stream from the seed (173, 173, 173))."""
    seed = np.array(S.SEED, np.int32)
    sigma = nb.sigma_of(snr, code.rate)
    cw = torch.zeros(code.N, dtype=torch.int32, device="cuda")
    return nb.Demodulate(code, nb.AWGNChannel_GPU(seed, sigma, code, cw, B), sigma)


def sample(B):
    return sorted({0, 1, B // 5, B // 3, B // 2 + 3, 2 * B // 3, B - 2, B - 1})


@pytest.mark.parametrize("cid", ["dv3_q16", "tail_q16"])
def test_persistent_form_on_the_new_shapes(nb, orc, monkeypatch, cid):
    """More frames than the chip holds workgroups: the kernels take their frames from a counter, and the per-lane state k_nb_ems
    keeps across frames (column offsets for dv <= 2, none for dv 3) must not leak from one frame into the next.  Against a code
    object created under NBLDPC_NO_PERSIST=1 on the whole batch, against the oracle on 8 frames."""
    case = S.BY_ID[cid]
    code = code_of(nb, case)
    monkeypatch.setenv("NBLDPC_NO_PERSIST", "1")
    plain = make_code(nb, case)
    monkeypatch.delenv("NBLDPC_NO_PERSIST")
    g = code.grids()
    assert g["persist_grid"] > 0 and g["pipe_grid"] == 0 and g["tmm_grid"] > 0 and g["tmm_grid_layered"] > 0
    oc = S.ocode(orc, case)
    runs = [("EMS", g["persist_grid"], "k_nb_ems", lambda c, L: nb.Decoding_EMS(c, L, 2, 2, S.MAX_ITER, want_state=True),
             lambda L: orc.nb_ems_decode(oc, L, 2, 2, S.MAX_ITER, want_state=True)),
            ("flooding trellis", g["tmm_grid"], "k_nb_tmm", lambda c, L: nb.Decoding_TMM(c, L, S.MAX_ITER, layered=False, want_state=True),
             lambda L: orc.nb_tmm_decode(oc, L, S.MAX_ITER, layered=False, want_state=True)),
            ("layered trellis", g["tmm_grid_layered"], "k_nb_tmm (layered)", lambda c, L: nb.Decoding_TMM(c, L, S.MAX_ITER, layered=True, want_state=True),
             lambda L: orc.nb_tmm_decode(oc, L, S.MAX_ITER, layered=True, want_state=True))]
    for what, grid, kernel, run, oracle in runs:
        B = grid + 37
        Lt = noisy_batch(nb, code, B, case.snr[1])
        a = run(code, Lt)
        assert code.last_kernel == kernel.replace(" (layered)", "") + (" (layered, frames from a counter)" if "layered" in kernel else " (frames from a counter)")
        b = run(plain, Lt)
        assert plain.last_kernel == kernel
        torch.cuda.synchronize()
        assert_same_call(a, b, what + " " + cid)
        assert len(set(a["iter_number"].cpu().tolist())) >= 3 and 0 < int(a["ok"].sum()) < B, what
        Lh = Lt.cpu().numpy()
        fr = sample(B)
        assert_frames(a, [oracle(Lh[f]) for f in fr], fr, what + " " + cid)


def test_workspace_slots_are_reused_at_gf4(nb, orc):
    """1 100 frames on the 1 024 workspace slots of k_nb_ems_hbm at q = 4 (a whole vector per float4 of the rank count): a
    workgroup's second frame starts from a slot its first one left behind.  Against the same frames in two calls of 550 (every frame
    in a fresh slot) and against the oracle on 8 frames."""
    case = S.BY_ID["hbm_q4"]
    code = code_of(nb, case)
    B = 1100
    Lt = noisy_batch(nb, code, B, case.snr[1])
    a = nb.Decoding_EMS(code, Lt, 2, 2, S.MAX_ITER, want_state=True)
    assert code.last_kernel == "k_nb_ems_hbm"
    halves = [nb.Decoding_EMS(code, Lt[i:i + 550].contiguous(), 2, 2, S.MAX_ITER, want_state=True) for i in (0, 550)]
    torch.cuda.synchronize()
    b = {k: torch.cat([h[k] for h in halves]) for k in a}
    assert_same_call(a, b, "1 100 frames against 2 x 550")
    assert len(set(a["iter_number"].cpu().tolist())) >= 3 and 0 < int(a["ok"].sum()) < B
    Lh = Lt.cpu().numpy()
    fr = sample(B) + [1024, 1099]  # frames behind the slot count
    oc = S.ocode(orc, case)
    assert_frames(a, [orc.nb_ems_decode(oc, Lh[f], 2, 2, S.MAX_ITER, want_state=True) for f in sorted(set(fr))], sorted(set(fr)), "hbm_q4")
