"""GPU tests of ordered-statistics reprocessing (include/bldpc.h): the kernels k_osd and k_osd_ws against the host statement
bldpc_decode_osd_host, exactly, on D, flips and scanned, on the shapes, batch sizes and inputs of tests/osd_cases.py
(tests/test_osd_cpu.py holds the host statement against the restatement on the same cases), every tier the case admits, with D_in NULL
and with about half the frames kept; a shipped code; D in place and apart; an empty and a full frame list; guard words
and each optional output alone; a caller's stream; scratch that grows and is reused; more listed frames than workspace slots; the other
decoders of a code object around an accepted and a refused call; the refusals the device makes; and Simulation_GPU(osd=True) against a
loop over the primitives, whole and in two shards, with osd=False giving the counters of the loop without reprocessing; and
Simulation_HARQ_GPU(osd=True), which reprocesses what stays unacknowledged and acknowledges nothing."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import DATA
from osd_cases import BATCHES, DIMS, WORKSPACE_DIMS, dims_id, kept_input, matrix, osd_input, processed_on_workspace

pytestmark = pytest.mark.gpu

BL = os.path.join(DATA, "bldpc")
KERNEL = {"lds": "k_osd", "workspace": "k_osd_ws"}


@pytest.fixture(scope="module")
def C():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_ldpc_amd
    return cuda_ldpc_amd


_codes, _host = {}, {}


def _code(C, dims, fresh=False):
    J, L, Z = dims
    if fresh:
        return C.BinaryCode.from_shifts(matrix(dims), J, L, Z)
    if dims not in _codes:
        _codes[dims] = C.BinaryCode.from_shifts(matrix(dims), J, L, Z)
    return _codes[dims]


def _app(dims, F):
    return np.array(osd_input(dims)[0][:, :F])  # a writable copy: torch takes no read-only array


def _want(C, dims, F, kept):
    """The host statement's result: computed once per case, shared among the tests.  kept: with kept_input(dims, F) as D_in."""
    key = (dims, F, kept)
    if key not in _host:
        J, L, Z = dims
        _host[key] = C.osd_host(matrix(dims), J, L, Z, _app(dims, F), kept_input(dims, F) if kept else None)
    return _host[key]


def _same(got, want, what):
    D, flips, scanned = got
    assert np.array_equal(flips.cpu().numpy(), want[1]), "flips: " + what
    assert np.array_equal(scanned.cpu().numpy(), want[2]), "scanned: " + what
    assert np.array_equal(D.cpu().numpy()[-1], want[0][-1]), "flag row: " + what
    assert np.array_equal(D.cpu().numpy(), want[0]), "D: " + what


def _tiers(C, dims):
    """The tiers to force, and the one AUTO takes."""
    auto = C.osd_plan_host(matrix(dims), *dims)["tier"]
    return (["lds"] if auto == "lds" else []) + ["workspace"], auto


def _both(C, dims, F, kept, tier="auto", code=None, apart=False, **kw):
    code = code or _code(C, dims)
    app = torch.from_numpy(_app(dims, F)).cuda()
    D = torch.from_numpy(kept_input(dims, F)).cuda() if kept else None
    out = torch.full((code.N + 1, F), -7, dtype=torch.int32, device="cuda") if apart else None
    r = C.LDPC_Decoder_OSD_GPU(code, app, D=D, tier=tier, out=out, **kw)
    torch.cuda.synchronize()
    assert code.last_kernel == KERNEL[_tiers(C, dims)[1] if tier == "auto" else tier]
    assert r[0] is (out if apart else D if kept else r[0])
    if apart and kept:
        assert np.array_equal(D.cpu().numpy(), kept_input(dims, F)), "D_in is read only"
    want = _want(C, dims, F, kept)
    _same(r, want, "%s F=%d kept=%s tier=%s apart=%s" % (dims_id(dims), F, kept, tier, apart))
    return r, want


@pytest.mark.parametrize("dims", DIMS, ids=dims_id)
def test_every_shape_matches_the_host_statement(C, dims):
    forced, auto = _tiers(C, dims)
    for F in BATCHES:
        for kept in ((True,) if dims == WORKSPACE_DIMS else (False, True)):  # WORKSPACE_DIMS: at most 8 processed frames a call
            for tier in forced + ["auto"]:
                for apart in ((False, True) if kept else (False,)):
                    _both(C, dims, F, kept, tier, apart=apart)
    assert len(processed_on_workspace()) == 8
    info = _code(C, dims).osd_info()
    assert info == C.osd_plan_host(matrix(dims), *dims) and info["tier"] == auto == ("workspace" if dims == WORKSPACE_DIMS else "lds")


def test_a_shipped_code(C):
    """J4_L24_Z96 on raw channel values of sigma 0.9, so every frame needs flips, on both tiers."""
    name, J, L, Z = "J4_L24_Z96_BlockH.txt", 4, 24, 96
    path = os.path.join(BL, name)
    H, _, _ = C.Get_H(path, J, L)
    code = C.BinaryCode.from_blockh(path, J, L, Z)
    F = 12
    y = (1.0 + 0.9 * np.random.default_rng(3).standard_normal((L * Z, F))).astype(np.float32)
    want = C.osd_host(H, J, L, Z, y)
    assert (want[1] > 0).all() and (want[2] > J * Z - 4).all()
    for tier in ("lds", "workspace", "auto"):
        r = C.LDPC_Decoder_OSD_GPU(code, torch.from_numpy(y).cuda(), tier=tier)
        torch.cuda.synchronize()
        _same(r, want, name + " " + tier)
        assert code.last_kernel == ("k_osd_ws" if tier == "workspace" else "k_osd")
    syn = C.Syndrome(code, r[0].clone(), into_flag_row=False)
    assert bool(syn["flag"].bool().all()), "every processed frame is a codeword"
    code.close()


def test_an_empty_frame_list_and_a_full_one(C):
    dims = (3, 7, 33)
    code = _code(C, dims)
    F = 37
    app = torch.from_numpy(_app(dims, F)).cuda()
    for tier in ("lds", "workspace"):
        Din = kept_input(dims, F)
        Din[-1] = np.arange(F) + 1  # every frame kept
        for apart in (False, True):
            D = torch.from_numpy(Din).cuda()
            out = torch.full_like(D, -7) if apart else None
            r = C.LDPC_Decoder_OSD_GPU(code, app, D=D, tier=tier, out=out)
            torch.cuda.synchronize()
            assert np.array_equal(r[0].cpu().numpy(), Din) and bool((r[1] == -1).all()) and bool((r[2] == 0).all())
        Din[-1] = 0  # every frame processed: the result of D_in = NULL
        r = C.LDPC_Decoder_OSD_GPU(code, app, D=torch.from_numpy(Din).cuda(), tier=tier)
        torch.cuda.synchronize()
        _same(r, _want(C, dims, F, False), "every frame listed, " + tier)


def test_guard_words_and_each_optional_output_alone(C):
    """The C entry point with D, flips and scanned inside guarded buffers; then flips alone, scanned alone and neither."""
    dims = (3, 7, 33)
    code = _code(C, dims)
    lib = C._lib.lib
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    G = 0x5A5A5A5A
    for F in (33, 37):
        app = torch.from_numpy(_app(dims, F)).cuda()
        nd = (code.N + 1) * F
        for kept in (False, True):
            want = _want(C, dims, F, kept)
            for tier in (1, 2):
                din = torch.from_numpy(kept_input(dims, F)).cuda() if kept else None
                dbuf = torch.full((nd + 64,), G, dtype=torch.int32, device="cuda")
                fbuf = torch.full((F + 8,), -3, dtype=torch.int32, device="cuda")
                sbuf = torch.full((F + 8,), -3, dtype=torch.int32, device="cuda")
                rc = lib.bldpc_decode_osd(code._h, ptr(app), ptr(din), F, tier, ptr(dbuf[32:]), ptr(fbuf[4:]), ptr(sbuf[4:]), st)
                torch.cuda.synchronize()
                assert rc == 0 and code.last_kernel == ("k_osd", "k_osd_ws")[tier - 1]
                d, fl, sc = dbuf.cpu().numpy(), fbuf.cpu().numpy(), sbuf.cpu().numpy()
                assert (d[:32] == G).all() and (d[32 + nd:] == G).all(), "a store outside D"
                assert np.array_equal(d[32:32 + nd].reshape(code.N + 1, F), want[0])
                assert (fl[:4] == -3).all() and (fl[4 + F:] == -3).all() and np.array_equal(fl[4:4 + F], want[1])
                assert (sc[:4] == -3).all() and (sc[4 + F:] == -3).all() and np.array_equal(sc[4:4 + F], want[2])
            for with_flips, with_scanned in ((True, False), (False, True), (False, False)):
                din = torch.from_numpy(kept_input(dims, F)).cuda() if kept else None
                D = torch.empty((code.N + 1, F), dtype=torch.int32, device="cuda")
                fl = torch.full((F,), -3, dtype=torch.int32, device="cuda")
                sc = torch.full((F,), -3, dtype=torch.int32, device="cuda")
                assert lib.bldpc_decode_osd(code._h, ptr(app), ptr(din), F, 0, ptr(D), ptr(fl) if with_flips else None,
                                            ptr(sc) if with_scanned else None, st) == 0
                torch.cuda.synchronize()
                assert np.array_equal(D.cpu().numpy(), want[0])
                assert np.array_equal(fl.cpu().numpy(), want[1] if with_flips else np.full(F, -3))
                assert np.array_equal(sc.cpu().numpy(), want[2] if with_scanned else np.full(F, -3))


def test_a_callers_stream(C):
    dims = (3, 9, 96)
    code = _code(C, dims)
    F = 37
    app = torch.from_numpy(_app(dims, F)).cuda()
    D = torch.from_numpy(kept_input(dims, F)).cuda()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())  # the uploads ran on the current stream
    r = C.LDPC_Decoder_OSD_GPU(code, app, D=D, stream=stream)
    stream.synchronize()
    assert r[0] is D
    _same(r, _want(C, dims, F, True), "stream=")


def test_scratch_that_grows_and_is_reused_by_a_smaller_call(C):
    dims = (3, 9, 96)
    code = _code(C, dims, fresh=True)
    for F, tier in ((37, "workspace"), (1, "lds"), (64, "workspace"), (33, "workspace"), (64, "lds"), (1, "workspace")):
        _both(C, dims, F, False, tier, code=code)
    code.close()


def test_more_listed_frames_than_workspace_slots(C):
    """The workspace shape with the slot count pinned to 3 (BLDPC_OSD_SLOTS, read when the plan is made) and 8 frames to process: every
    workgroup takes frame after frame from the list, and its slot, keys and bitmaps are reused."""
    dims = WORKSPACE_DIMS
    os.environ["BLDPC_OSD_SLOTS"] = "3"
    try:
        code = _code(C, dims, fresh=True)
        assert code.osd_info()["slots"] == 3
    finally:
        del os.environ["BLDPC_OSD_SLOTS"]
    _, want = _both(C, dims, 64, True, code=code)
    assert (want[1] >= 0).sum() == 8
    assert code.osd_info()["slots"] == 3 and _code(C, dims).osd_info()["slots"] > 3
    code.close()
    small = (3, 9, 96)  # and with every frame listed, on a shape that a frame costs little
    os.environ["BLDPC_OSD_SLOTS"] = "2"
    try:
        code = _code(C, small, fresh=True)
        assert code.osd_info(tier="workspace")["slots"] == 2
    finally:
        del os.environ["BLDPC_OSD_SLOTS"]
    _both(C, small, 64, False, "workspace", code=code)
    code.close()


def _others(C, c, yy):
    from test_erasure_gpu import _others as rest
    return rest(C, c, yy)


def test_other_decoders_unchanged_around_an_accepted_and_a_refused_call(C):
    from cuda_ldpc_amd._lib import LdpcError
    dims = WORKSPACE_DIMS
    code = _code(C, dims, fresh=True)
    F = 37
    y = torch.from_numpy(_app(dims, F)).cuda()
    before = _others(C, code, y)
    assert len(before) == 14
    _both(C, dims, F, True, code=code)
    _both(C, dims, F, True, code=code, apart=True)
    D = torch.full((code.N + 1, F), -7, dtype=torch.int32, device="cuda")
    kernel, said = code.last_kernel, []
    for _ in range(2):
        with pytest.raises(LdpcError, match=r"\(-5\): .*BLDPC_ML_LDS") as err:
            C.LDPC_Decoder_OSD_GPU(code, y, tier="lds", out=D)
        said.append(str(err.value))
    torch.cuda.synchronize()
    assert said[0] == said[1] and code.last_kernel == kernel and bool((D == -7).all()), "a refused call launches nothing"
    after = _others(C, code, y)
    assert all(torch.equal(x, z) for x, z in zip(before, after))
    _both(C, dims, F, True, code=code)
    code.close()


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

    def raw(F=F, app=app, D=D, tier=0):
        out = []
        for _ in range(2):
            rc = lib.bldpc_decode_osd(code._h, ptr(app), None, F, tier, ptr(D), None, None, st)
            out.append((rc, lib.bldpc_last_error().decode() if rc else ""))
        assert out[0] == out[1]
        return out[0]

    who = "bldpc_decode_osd"
    assert raw() == (0, "")
    assert raw(F=0) == (-1, who + ": F=0 must be positive") and raw(F=-2)[0] == -1
    assert raw(app=None) == (-1, who + ": null app") and raw(D=None) == (-1, who + ": null D")
    assert raw(tier=3) == (-1, who + ": unknown tier 3") and raw(tier=-1)[0] == -1
    assert lib.bldpc_decode_osd(None, ptr(app), None, F, 0, ptr(D), None, None, st) == -1
    for bad in (dict(app=app.double()), dict(app=app[:-1]), dict(app=app.cpu()), dict(D=torch.empty((N, F), dtype=torch.int32, device="cuda")),
                dict(out=torch.empty((N + 1, F + 1), dtype=torch.int32, device="cuda")), dict(tier="fast")):
        with pytest.raises(ValueError):
            C.LDPC_Decoder_OSD_GPU(code, **dict(dict(app=app), **bad))
    name, J, L, Z = "J4_L24_Z96_BlockH.txt", 4, 24, 96
    H, wc, wv = C.Get_H(os.path.join(BL, name), J, L)
    table = C.BinaryCode.from_table(J, L, Z, wc, wv, C.Transform_H(H, J, L, Z, wc, wv))
    said = []
    for _ in range(2):
        with pytest.raises(LdpcError, match=r"\(-5\): .*address table") as e:
            C.LDPC_Decoder_OSD_GPU(table, torch.ones((table.N, F), device="cuda"))
        said.append(str(e.value))
    assert said[0] == said[1]
    with pytest.raises(LdpcError, match=r"\(-5\): .*address table"):
        table.osd_info()
    pon = C.BinaryCode.from_blockh(os.path.join(BL, "PON_LDPC.txt"), 12, 69, 256)  # the keys of 17 664 positions fit neither tier
    for tier in ("auto", "lds", "workspace"):
        with pytest.raises(LdpcError, match=r"\(-5\): .*sort keys"):
            C.LDPC_Decoder_OSD_GPU(pon, torch.ones((pon.N, 2), device="cuda"), tier=tier)
    pon.close()
    torch.cuda.synchronize()
    _both(C, dims, 37, False)  # the code object decodes as before


# ---- the driver -------------------------------------------------------------------------------------------------------------------------
class _Rank:
    """One rank of a world of `world` without a process group: the all-reduce is the sum the test makes."""

    def __init__(self, rank, world):
        self.rank, self.world = rank, world

    def is_initialized(self):
        return True

    def get_rank(self):
        return self.rank

    def get_world_size(self):
        return self.world

    def all_reduce(self, t):
        return t


def _counters(SIM):
    return [SIM.num_Error_Frames, SIM.num_Error_Bits, SIM.Total_Iteration, SIM.num_False_Frames, SIM.num_Alarm_Frames]


def test_simulation_with_and_without_reprocessing(C):
    """Two batches of 128 random codewords on J4_L24_Z96 at 2.0 dB, ten iterations of layered min-sum: the counters of
    Simulation_GPU(osd=True) recomputed from the primitives in a plain loop, then as the sum over the ranks of a world of 2; osd=False
    gives the counters of the same loop without the reprocessing call."""
    from cuda_ldpc_amd.simulation import Simulation_GPU
    J, L, Z = 4, 24, 96
    code = C.BinaryCode.from_blockh(os.path.join(BL, "J4_L24_Z96_BlockH.txt"), J, L, Z)
    N, K = code.N, code.K
    F, batches, maxIT, pn_seed, alpha = 128, 2, 10, 4242, 0.75
    sigma = C.sigma_of(2.0, 1, K / N)
    kw = dict(Num_Frames_OneTime=F, maxIT=maxIT, exit_mode=C.EXIT_PER_FRAME, max_batches=batches, log=None, PN_Message=1, pn_seed=pn_seed,
              schedule="layered", alpha=alpha, leastTestFrames=10 ** 9)

    def count(D, cw, it):
        errs = (D[:K] != cw[:K]).sum(0)
        ok = D[N] != 0
        return np.array([np.sum((errs != 0) | ~ok), errs.sum(), it.sum(), np.sum((errs != 0) & ok), np.sum((errs == 0) & ~ok)], np.int64)

    seed, plain, with_osd, osd = np.array([173, 173, 173], np.int32), np.zeros(5, np.int64), np.zeros(5, np.int64), np.zeros(2, np.int64)
    for b in range(batches):
        cw = C.PN_CodeWords(code, pn_seed, F, first_frame=b * F)
        y = C.AWGNChannel_CPU(seed, sigma, N, F, CodeWord=cw.cpu().numpy())
        r = C.LDPC_Decoder_Layered_GPU(code, torch.from_numpy(y).cuda(), max_iter=maxIT, alpha=alpha, exit_mode=C.EXIT_PER_FRAME,
                                       stop_rule=C.STOP_SYNDROME, want_app=True)
        cwn, it = cw.cpu().numpy(), r["iters"].cpu().numpy()
        plain += count(r["D"].cpu().numpy(), cwn, it)
        D2, flips, _ = C.LDPC_Decoder_OSD_GPU(code, r["app"], D=r["D"])
        D2, flips = D2.cpu().numpy(), flips.cpu().numpy()
        with_osd += count(D2, cwn, it)
        osd += [np.sum(flips >= 0), np.sum((flips >= 0) & (D2[:N] == cwn).all(0))]
    SIM, seed1 = C.SimCounters(), np.array([173, 173, 173], np.int32)
    Simulation_GPU(code, seed1, sigma, SIM, osd=True, **kw)
    assert code.last_kernel == "k_osd"
    print("layered %s, with reprocessing %s, reprocessed %d, of them correct %d" % (plain.tolist(), with_osd.tolist(), osd[0], osd[1]))
    assert SIM.num_Frames == F * batches and _counters(SIM) == with_osd.tolist() and np.array_equal(seed1, seed)
    assert [SIM.num_OSD_Frames, SIM.num_OSD_Correct] == osd.tolist() and osd[0] == plain[0] - plain[3] > 0
    assert with_osd[4] == 0 and with_osd[0] == with_osd[3], "every frame comes out a codeword: an error is an undetected one"
    total, total_osd = np.zeros(5, np.int64), np.zeros(2, np.int64)
    for rank in range(2):
        part, seed2 = C.SimCounters(), np.array([173, 173, 173], np.int32)
        Simulation_GPU(code, seed2, sigma, part, osd=True, dist=_Rank(rank, 2), **kw)
        total += _counters(part)
        total_osd += [part.num_OSD_Frames, part.num_OSD_Correct]
        assert np.array_equal(seed2, seed)
    assert total.tolist() == with_osd.tolist() and total_osd.tolist() == osd.tolist()
    for more in (dict(), dict(osd=False)):
        SIM, seed3 = C.SimCounters(), np.array([173, 173, 173], np.int32)
        Simulation_GPU(code, seed3, sigma, SIM, **dict(kw, **more))
        assert _counters(SIM) == plain.tolist() and np.array_equal(seed3, seed) and SIM.num_OSD_Frames == 0
    for bad in (dict(schedule="flooding", exit_mode=C.EXIT_FIXED, alpha=1.0), dict(stop_rule=C.STOP_PREFIX, exit_mode=C.EXIT_FIXED),
                dict(schedule="hard", alpha=1.0)):
        with pytest.raises(ValueError, match="osd"):
            Simulation_GPU(code, np.array([173, 173, 173], np.int32), sigma, C.SimCounters(), osd=True, **dict(kw, **bad))
    code.close()


def test_harq_reprocesses_what_stays_unacknowledged_and_acknowledges_nothing(C):
    """Simulation_HARQ_GPU on J4_L24_Z96 with the first two transmissions of test_harq_gpu.py and three layered iterations, so that frames
    stay unacknowledged: osd=True leaves every counter of osd=False as it is, reprocesses exactly the frames never acknowledged, hands
    keep_D codewords with flag 1 in their columns and the other columns unchanged; decoding only the unacknowledged frames (compact)
    and the whole batch give the same words, so the app of a compacted decode is scattered back where it belongs."""
    import qc_variant_cases as Q
    from cuda_ldpc_amd.simulation import HarqCounters, Simulation_HARQ_GPU
    from test_harq_gpu import SHORT_LLR, SIM_PUNCT, SIM_RVS, SIM_SHORT, SIM_SNR
    path, _, J, L, Z = Q.matrix(("shipped", "J4_L24_Z96"))
    code = C.BinaryCode.from_blockh(path, J, L, Z)
    N = code.N
    rvs = [C.RateMatch.circular(N, SIM_SHORT, SIM_PUNCT, k0, E) for k0, E in SIM_RVS[:2]]
    F, batches = 128, 2
    kw = dict(Num_Frames_OneTime=F, max_batches=batches, log=None, short_llr=SHORT_LLR, leastTestFrames=10 ** 9, PN_Message=1, pn_seed=31337, alpha=0.75,
              maxIT=3, exit_mode=C.EXIT_PER_FRAME, schedule="layered", stop_rule=C.STOP_SYNDROME)

    def run(**more):
        SIM, seed, Ds = HarqCounters(), np.array([173, 173, 173], np.int32), []
        Simulation_HARQ_GPU(code, seed, C.sigma_of(SIM_SNR), SIM, rvs, keep_D=Ds, **dict(kw, **more))
        return SIM, seed, Ds

    plain, seed0, D0 = run()
    assert 0 < plain.never_acked < F * batches and plain.osd_frames == 0
    for compact in (True, False):
        SIM, seed, Ds = run(osd=True, compact=compact)
        assert SIM == plain and np.array_equal(seed, seed0), "the acknowledgement stays the decoder's flag"
        assert SIM.osd_frames == plain.never_acked and 0 <= SIM.osd_correct <= SIM.osd_frames
        for D, Dp in zip(Ds, D0):
            acked = Dp[N] != 0
            assert bool((D[N] == 1).all()) and torch.equal(D[:, acked], Dp[:, acked])
            assert bool(C.Syndrome(code, D.clone(), into_flag_row=False)["flag"].bool().all()), "every frame is a codeword now"
        if compact:
            first = Ds
        else:
            assert all(torch.equal(a, b) for a, b in zip(first, Ds))
    print("HARQ, two transmissions, three iterations: %d of %d never acknowledged, %d of them equal to the word sent after reprocessing" % (
        plain.never_acked, F * batches, SIM.osd_correct))
    with pytest.raises(ValueError, match="osd"):
        run(osd=True, schedule="flooding", stop_rule=None, exit_mode=C.EXIT_FIXED)
    code.close()
