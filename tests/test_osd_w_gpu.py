"""GPU tests of reprocessing of order 1 and 2 (include/bldpc.h): the kernels k_osd_w and k_osd_w_ws against the host statement
bldpc_decode_osd_w_host, exactly, on D, flips, scanned, picked and the metric bits, on the shapes, batch sizes, inputs and parameter
sets of tests/osd_w_cases.py (tests/test_osd_w_cpu.py holds the host statement against the restatement on the same cases), every tier
the case admits, with D_in NULL and with about half the frames kept, in place and apart; order 0 against LDPC_Decoder_OSD_GPU; the
kernel names; a second call on the same scratch; guard words and each optional output alone; the refusals the device makes; and
Simulation_GPU(osd=True, osd_order=2, osd_lambda=12) against a loop over the primitives."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import DATA
from osd_w_cases import DIMS, WORKSPACE_DIMS, batches, dims_id, kept_w_input, matrix, metric_bits, osd_w_input, params, processed_w

pytestmark = pytest.mark.gpu

BL = os.path.join(DATA, "bldpc")
KERNEL = {"lds": "k_osd_w", "workspace": "k_osd_w_ws"}


@pytest.fixture(scope="module")
def C():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_ldpc_amd
    return cuda_ldpc_amd


_codes, _host = {}, {}


def _code(C, dims):
    J, L, Z = dims
    if dims not in _codes:
        _codes[dims] = C.BinaryCode.from_shifts(matrix(dims), J, L, Z)
    return _codes[dims]


def _app(dims, F):
    return np.array(osd_w_input(dims)[0][:, :F])  # a writable copy: torch takes no read-only array


def _want(C, dims, F, kept, order, lam):
    """The host statement's result: computed once per case, shared among the tests."""
    key = (dims, F, kept, order, lam)
    if key not in _host:
        J, L, Z = dims
        _host[key] = C.osd_host(matrix(dims), J, L, Z, _app(dims, F), kept_w_input(dims, F) if kept else None, order=order, lam=lam, want_metric=True)
    return _host[key]


def _same(got, want, what):
    D, flips, scanned, picked, metric = (t.cpu().numpy() for t in got)
    done = want[1] >= 0
    assert np.array_equal(flips, want[1]), "flips: " + what
    assert np.array_equal(scanned, want[2]), "scanned: " + what
    assert np.array_equal(picked, want[3]), "picked: " + what
    assert np.array_equal(metric_bits(metric)[done], metric_bits(want[4])[done]), "metric bits: " + what
    assert np.array_equal(D, want[0]), "D: " + what


def _tiers(C, dims, order):
    """The tiers to force, and the one AUTO takes."""
    auto = C.osd_plan_host(matrix(dims), *dims, order=order)["tier"]
    return (["lds"] if auto == "lds" else []) + ["workspace"], auto


def _both(C, dims, F, kept, order, lam, tier="auto", apart=False):
    code = _code(C, dims)
    app = torch.from_numpy(_app(dims, F)).cuda()
    D = torch.from_numpy(kept_w_input(dims, F)).cuda() if kept else None
    out = torch.full((code.N + 1, F), -7, dtype=torch.int32, device="cuda") if apart else None
    r = C.LDPC_Decoder_OSD_GPU(code, app, D=D, tier=tier, out=out, order=order, lam=lam, want_metric=True)
    torch.cuda.synchronize()
    assert code.last_kernel == KERNEL[_tiers(C, dims, order)[1] if tier == "auto" else tier]
    assert r[0] is (out if apart else D if kept else r[0])
    if apart and kept:
        assert np.array_equal(D.cpu().numpy(), kept_w_input(dims, F)), "D_in is read only"
    want = _want(C, dims, F, kept, order, lam)
    _same(r, want, "%s F=%d kept=%s order=%d lambda=%d tier=%s apart=%s" % (dims_id(dims), F, kept, order, lam, tier, apart))
    return r, want


CASES = [(dims, order, lam, F) for dims in DIMS for order, lam in params(dims) for F in batches(dims)]  # a case a batch: lambda = N costs seconds


@pytest.mark.parametrize("dims,order,lam,F", CASES, ids=lambda v: dims_id(v) if isinstance(v, tuple) else str(v))
def test_every_shape_matches_the_host_statement(C, dims, order, lam, F):
    forced, auto = _tiers(C, dims, order)
    assert auto == ("workspace" if dims == WORKSPACE_DIMS else "lds")
    for kept in ((True,) if dims == WORKSPACE_DIMS else (False, True)):  # WORKSPACE_DIMS: at most 4 processed frames a call
        for tier in forced + ["auto"]:
            for apart in ((False, True) if kept else (False,)):
                _both(C, dims, F, kept, order, lam, tier, apart=apart)
    info = _code(C, dims).osd_info(order=order)
    assert info == C.osd_plan_host(matrix(dims), *dims, order=order) and info["tier"] == auto
    assert len(processed_w()) == 4


@pytest.mark.parametrize("dims", [(3, 7, 33), WORKSPACE_DIMS], ids=dims_id)
def test_order_0_is_the_call_of_today_and_a_second_call_repeats(C, dims):
    code = _code(C, dims)
    F = 37
    app = torch.from_numpy(_app(dims, F)).cuda()
    for tier in _tiers(C, dims, 0)[0]:
        old = C.LDPC_Decoder_OSD_GPU(code, app, D=torch.from_numpy(kept_w_input(dims, F)).cuda(), tier=tier)
        torch.cuda.synchronize()
        assert len(old) == 3 and code.last_kernel == {"lds": "k_osd", "workspace": "k_osd_ws"}[tier]
        new = C.LDPC_Decoder_OSD_GPU(code, app, D=torch.from_numpy(kept_w_input(dims, F)).cuda(), tier=tier, want_metric=True)
        torch.cuda.synchronize()
        assert len(new) == 5 and code.last_kernel == KERNEL[tier]
        assert all(torch.equal(x, z) for x, z in zip(old, new[:3])) and bool((new[3] == -1).all())
        for order, lam in params(dims)[1:]:
            first, _ = _both(C, dims, F, True, order, lam, tier)
            again, _ = _both(C, dims, F, True, order, lam, tier)
            done = first[1] >= 0
            assert all(torch.equal(x, z) for x, z in zip(first[:4], again[:4])) and torch.equal(first[4][done].view(torch.int32), again[4][done].view(torch.int32))


def test_guard_words_and_each_optional_output_alone(C):
    """The C entry point with every output inside guarded buffers; then each optional output left out in turn."""
    dims = (3, 7, 33)
    code = _code(C, dims)
    lib = C._lib.lib
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    G = 0x5A5A5A5A
    F, order, lam = 37, 2, 12
    app = torch.from_numpy(_app(dims, F)).cuda()
    nd = (code.N + 1) * F
    for kept in (False, True):
        want = _want(C, dims, F, kept, order, lam)
        done = want[1] >= 0
        for tier in (1, 2):
            din = torch.from_numpy(kept_w_input(dims, F)).cuda() if kept else None
            dbuf = torch.full((nd + 64,), G, dtype=torch.int32, device="cuda")
            fbuf, sbuf, mbuf = (torch.full((F + 8,), -3, dtype=torch.int32, device="cuda") for _ in range(3))
            pbuf = torch.full((2 * F + 8,), -3, dtype=torch.int32, device="cuda")
            rc = lib.bldpc_decode_osd_w(code._h, ptr(app), ptr(din), F, tier, order, lam, ptr(dbuf[32:]), ptr(fbuf[4:]), ptr(sbuf[4:]), ptr(pbuf[4:]),
                                        ptr(mbuf[4:]), st)
            torch.cuda.synchronize()
            assert rc == 0 and code.last_kernel == ("k_osd_w", "k_osd_w_ws")[tier - 1]
            d, fl, sc, pk, me = (t.cpu().numpy() for t in (dbuf, fbuf, sbuf, pbuf, mbuf))
            assert (d[:32] == G).all() and (d[32 + nd:] == G).all(), "a store outside D"
            assert np.array_equal(d[32:32 + nd].reshape(code.N + 1, F), want[0])
            assert (fl[:4] == -3).all() and (fl[4 + F:] == -3).all() and np.array_equal(fl[4:4 + F], want[1])
            assert (sc[:4] == -3).all() and (sc[4 + F:] == -3).all() and np.array_equal(sc[4:4 + F], want[2])
            assert (pk[:4] == -3).all() and (pk[4 + 2 * F:] == -3).all() and np.array_equal(pk[4:4 + 2 * F].reshape(2, F), want[3])
            assert (me[:4] == -3).all() and (me[4 + F:] == -3).all() and (me[4:4 + F][~done] == -3).all(), "metric of a kept frame is unwritten"
            assert np.array_equal(metric_bits(me[4:4 + F].view(np.float32))[done], metric_bits(want[4])[done])
        for leave in range(4):
            din = torch.from_numpy(kept_w_input(dims, F)).cuda() if kept else None
            D = torch.empty((code.N + 1, F), dtype=torch.int32, device="cuda")
            outs = [torch.full((F,), -3, dtype=torch.int32, device="cuda"), torch.full((F,), -3, dtype=torch.int32, device="cuda"),
                    torch.full((2, F), -3, dtype=torch.int32, device="cuda"), torch.full((F,), -3.0, dtype=torch.float32, device="cuda")]
            given = [None if k == leave else ptr(t) for k, t in enumerate(outs)]
            assert lib.bldpc_decode_osd_w(code._h, ptr(app), ptr(din), F, 0, order, lam, ptr(D), *given, st) == 0
            torch.cuda.synchronize()
            assert np.array_equal(D.cpu().numpy(), want[0])
            for k, t in enumerate(outs[:3]):
                assert np.array_equal(t.cpu().numpy(), np.full(t.shape, -3) if k == leave else want[1 + k])
            assert bool((outs[3] == -3.0).all()) if leave == 3 else np.array_equal(metric_bits(outs[3].cpu().numpy())[done], metric_bits(want[4])[done])


def test_refusals_on_the_device(C):
    from cuda_ldpc_amd._lib import LdpcError
    dims = (3, 9, 96)
    code = _code(C, dims)
    F, N = 4, code.N
    app = torch.ones((N, F), device="cuda")
    lib = C._lib.lib
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    D = torch.empty((N + 1, F), dtype=torch.int32, device="cuda")
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def raw(F=F, app=app, D=D, tier=0, order=1, lam=0):
        out = []
        for _ in range(2):
            rc = lib.bldpc_decode_osd_w(code._h, ptr(app), None, F, tier, order, lam, ptr(D), None, None, None, None, st)
            out.append((rc, lib.bldpc_last_error().decode() if rc else ""))
        assert out[0] == out[1]
        return out[0]

    who = "bldpc_decode_osd_w"
    assert raw() == (0, "")
    assert raw(F=0) == (-1, who + ": F=0 must be positive") and raw(app=None) == (-1, who + ": null app") and raw(D=None) == (-1, who + ": null D")
    assert raw(tier=3) == (-1, who + ": unknown tier 3")
    assert raw(order=3) == (-1, who + ": order 3 outside 0 .. 2") and raw(order=-1)[0] == -1
    assert raw(order=2, lam=-1) == (-1, who + ": lambda=-1 must not be negative")
    assert lib.bldpc_decode_osd_w(None, ptr(app), None, F, 0, 1, 0, ptr(D), None, None, None, None, st) == -1
    info = np.zeros(4, np.int32)
    assert lib.bldpc_osd_w_info(code._h, 0, 3, info.ctypes.data_as(ctypes.c_void_p)) == -1
    assert lib.bldpc_osd_w_info(code._h, 0, 2, None) == -1
    pon = C.BinaryCode.from_blockh(os.path.join(BL, "PON_LDPC.txt"), 12, 69, 256)  # the keys of 17 664 positions fit neither tier
    for tier in ("auto", "lds", "workspace"):
        with pytest.raises(LdpcError, match=r"\(-5\): .*sort keys"):
            C.LDPC_Decoder_OSD_GPU(pon, torch.ones((pon.N, 2), device="cuda"), tier=tier, order=2, lam=4)
    with pytest.raises(LdpcError, match=r"\(-5\): .*sort keys"):
        pon.osd_info(order=1)
    pon.close()
    torch.cuda.synchronize()
    _both(C, dims, 37, False, 2, 12)  # the code object decodes as before


# ---- the driver -------------------------------------------------------------------------------------------------------------------------
def test_simulation_at_order_2(C):
    """Two batches of 128 random codewords on J4_L24_Z96 at 2.0 dB, ten iterations of layered min-sum (the setting of test_osd_gpu.py):
    the counters of Simulation_GPU(osd=True, osd_order=2, osd_lambda=12) recomputed from the primitives in a plain loop."""
    from cuda_ldpc_amd.simulation import Simulation_GPU
    J, L, Z = 4, 24, 96
    code = C.BinaryCode.from_blockh(os.path.join(BL, "J4_L24_Z96_BlockH.txt"), J, L, Z)
    N, K = code.N, code.K
    F, batches_, maxIT, pn_seed, alpha = 128, 2, 10, 4242, 0.75
    sigma = C.sigma_of(2.0, 1, K / N)
    kw = dict(Num_Frames_OneTime=F, maxIT=maxIT, exit_mode=C.EXIT_PER_FRAME, max_batches=batches_, log=None, PN_Message=1, pn_seed=pn_seed,
              schedule="layered", alpha=alpha, leastTestFrames=10 ** 9)

    def count(D, cw, it):
        errs = (D[:K] != cw[:K]).sum(0)
        ok = D[N] != 0
        return np.array([np.sum((errs != 0) | ~ok), errs.sum(), it.sum(), np.sum((errs != 0) & ok), np.sum((errs == 0) & ~ok)], np.int64)

    seed, with_osd, osd = np.array([173, 173, 173], np.int32), np.zeros(5, np.int64), np.zeros(2, np.int64)
    for b in range(batches_):
        cw = C.PN_CodeWords(code, pn_seed, F, first_frame=b * F)
        y = C.AWGNChannel_CPU(seed, sigma, N, F, CodeWord=cw.cpu().numpy())
        r = C.LDPC_Decoder_Layered_GPU(code, torch.from_numpy(y).cuda(), max_iter=maxIT, alpha=alpha, exit_mode=C.EXIT_PER_FRAME,
                                       stop_rule=C.STOP_SYNDROME, want_app=True)
        cwn, it = cw.cpu().numpy(), r["iters"].cpu().numpy()
        D2, flips, _, picked, _ = C.LDPC_Decoder_OSD_GPU(code, r["app"], D=r["D"], order=2, lam=12)
        D2, flips = D2.cpu().numpy(), flips.cpu().numpy()
        with_osd += count(D2, cwn, it)
        osd += [np.sum(flips >= 0), np.sum((flips >= 0) & (D2[:N] == cwn).all(0))]
    SIM, seed1 = C.SimCounters(), np.array([173, 173, 173], np.int32)
    Simulation_GPU(code, seed1, sigma, SIM, osd=True, osd_order=2, osd_lambda=12, **kw)
    assert code.last_kernel == "k_osd_w"
    print("with reprocessing at (2, 12) %s, reprocessed %d, of them correct %d" % (with_osd.tolist(), osd[0], osd[1]))
    assert SIM.num_Frames == F * batches_ and np.array_equal(seed1, seed) and osd[0] > 0
    assert [SIM.num_Error_Frames, SIM.num_Error_Bits, SIM.Total_Iteration, SIM.num_False_Frames, SIM.num_Alarm_Frames] == with_osd.tolist()
    assert [SIM.num_OSD_Frames, SIM.num_OSD_Correct] == osd.tolist()
    with pytest.raises(ValueError, match="osd_order"):
        Simulation_GPU(code, np.array([173, 173, 173], np.int32), sigma, C.SimCounters(), osd_order=1, **kw)
    code.close()
