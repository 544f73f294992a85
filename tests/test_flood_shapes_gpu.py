"""GPU tests of the flooding decoders (bldpc_decode, bldpc_decode_per_frame, bldpc_decode_normalised, bldpc_decode_statistic,
bldpc_statistic) on the generated codes of tests/flood_shape_cases.py: the table kernels where they are the only path (Z = 1, Z
below 32, Z and N no multiple of 32 or 4, lifting sizes without an entry, block columns of weight 16, 1 and 0, block rows of
weight 26 and 2, M and N above the grid cap, the level schedule of an as-written table, two workgroups in x, a misaligned input)
and the generic compressed-state tier at both sides of its acceptance bounds.  Every comparison is exact: hard bits, flag row,
iteration counts, flag histories, a-posteriori bit patterns and the five counters, against the CPU oracle (alpha 0.75: against
bldpc_decode_normalised_host), which tests/test_flood_shapes_cpu.py holds against the numpy restatements on the same cases."""
import numpy as np
import pytest
import torch

import flood_shape_cases as FS
from flood_shape_cases import BATCHES, F_RAMP, GRID_CAP, LARGE, MAXIT, SHAPES, shape_id

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def C():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_ldpc_amd
    return cuda_ldpc_amd


_codes, _dev, _host = {}, {}, {}


def _code(C, s):
    if s not in _codes:
        _codes[s] = FS.make_code(C, s)
    return _codes[s]


def _t(y):
    """The device copy of a shared host input (kept with the array it was made from)."""
    if id(y) not in _dev:
        _dev[id(y)] = (y, torch.from_numpy(y.copy()).cuda())
    return _dev[id(y)][1]


def _kernels(C, s):
    return (C.KERNEL_AUTO, C.KERNEL_TABLE) + ((C.KERNEL_QC_LDS,) if s.landing else ())


def _ran(C, code, s, kernel, F, norm=False):
    """The kernel the call must have run on: the table kernels by batch size, or the shape's fused entry."""
    if kernel == C.KERNEL_TABLE or s.landing is None:
        want = ("table_vec4" if F % 4 == 0 else "table_vec1") + ("_norm" if norm else "")
        assert code.last_kernel == want, "%s F=%d ran %s" % (shape_id(s), F, code.last_kernel)
    else:
        assert code.last_kernel.startswith("qc_lds_" + s.landing + "<") and code.last_kernel.endswith("_norm") == norm, code.last_kernel


def _same(code, r, want, what, its=None):
    N = code.N
    D = r["D"].cpu().numpy()
    if "iters" in want:
        assert np.array_equal(r["iters"].cpu().numpy(), want["iters"]), "iters: " + what
    else:
        assert r["iteraTime"] == want["it"], "iteraTime %d, not %d: %s" % (r["iteraTime"], want["it"], what)
    assert np.array_equal(D[N], want["D"][N]), "flag row: " + what
    assert np.array_equal(D[:N], want["D"][:N]), "hard bits: " + what
    if r.get("app") is not None:
        assert np.array_equal(r["app"].cpu().numpy().view(np.uint32), want["app"].view(np.uint32)), "a-posteriori bits: " + what
    if r.get("flag_hist") is not None:
        mask = np.uint64((1 << min(its, 64)) - 1)
        assert np.array_equal(r["flag_hist"].cpu().numpy().view(np.uint64) & mask, want["flag_hist"] & mask), "flag history: " + what


def _decode(C, code, y, **kw):
    r = C.LDPC_Decoder_GPU(code, _t(y), want_app=True, **kw)
    torch.cuda.synchronize()
    return r


def _host_norm(C, s, key, y, **kw):
    k = (s, key, y.shape[1], tuple(sorted(kw.items())))
    if k not in _host:
        _host[k] = C.normalised_host(FS.matrix_of(s), s.J, s.L, s.Z, y, **kw)
    return _host[k]


def _fixed(C, orc, s, kernel, key, y, its, length=0, alpha=None, code=None):
    code, F = code or _code(C, s), y.shape[1]
    what = "%s %s F=%d kernel=%d fixed %d length=%d alpha=%s" % (shape_id(s), key, F, kernel, its, length, alpha)
    if alpha is None:
        r = _decode(C, code, y, max_iter=its, length=length, exit_mode=C.EXIT_FIXED, kernel=kernel, want_flag_hist=True)
    else:
        r = _decode(C, code, y, max_iter=its, length=length, exit_mode=C.EXIT_FIXED, kernel=kernel, alpha=alpha)
    if alpha is None or alpha == 1.0:
        want = FS.want_fixed(orc, s, key, y, its, length)
    else:
        h = _host_norm(C, s, key, y, max_iter=its, alpha=alpha, length=length)
        want = dict(D=h["D"], app=h["app"], it=its)
    _same(code, r, want, what, its)
    _ran(C, code, s, kernel, F, alpha is not None)
    return r


def _per_frame(C, orc, s, kernel, key, y, length=0, alpha=None, max_iter=MAXIT, code=None):
    code, F = code or _code(C, s), y.shape[1]
    what = "%s %s F=%d kernel=%d per-frame length=%d alpha=%s" % (shape_id(s), key, F, kernel, length, alpha)
    r = _decode(C, code, y, max_iter=max_iter, length=length, exit_mode=C.EXIT_PER_FRAME, kernel=kernel, alpha=alpha)
    if alpha is None or alpha == 1.0:
        want = FS.want_per_frame(orc, s, key, y, max_iter, length)
    else:
        want = _host_norm(C, s, key, y, max_iter=max_iter, alpha=alpha, length=length, exit_mode=C.EXIT_PER_FRAME)
    _same(code, r, want, what)
    _ran(C, code, s, kernel, F, alpha is not None)
    return r


def _global(C, orc, s, kernel, F, length=0, code=None):
    code = code or _code(C, s)
    key, y = FS.global_ramp(s, F)
    want = FS.want_global(orc, s, key, y, length=length)
    r = _decode(C, code, y, max_iter=MAXIT, length=length, exit_mode=C.EXIT_BATCH_GLOBAL, kernel=kernel, want_flag_hist=True)
    _same(code, r, want, "%s %s F=%d kernel=%d batch-global length=%d" % (shape_id(s), key, F, kernel, length), want["it"])
    _ran(C, code, s, kernel, F)
    return want["it"]


@pytest.mark.parametrize("s", SHAPES, ids=shape_id)
def test_every_shape_in_every_mode(C, orc, s):
    code = _code(C, s)
    N, large = code.N, s[:3] == LARGE
    variants = C.qc_variants()
    assert (code.N, code.M, code.K) == (s.L * s.Z, s.J * s.Z, (s.L - s.J) * s.Z)
    if s.landing is None:
        assert code.qc_variant == -1
    else:
        assert variants[code.qc_variant]["tag"] == s.landing and code.qc_variant == C.qc_plan_host(FS.matrix_of(s), s.Z).variant
    if large:
        assert code.levels == 1 and code.M > GRID_CAP and code.N > GRID_CAP, "both stride loops must take a second trip"
    if s.edit == "literal":
        assert code.levels > 1 and code.frames_per_wg == 0
    else:
        assert code.levels == 1
    stops = set()
    for kernel in _kernels(C, s):
        for F in BATCHES:
            y = FS.ramp(s, F)
            for its in FS.FIXED_ITS:
                _fixed(C, orc, s, kernel, "ramp", y, its)
            if large:
                continue
            stops.add(_global(C, orc, s, kernel, F))
            for length in FS.lengths_of(s):
                _fixed(C, orc, s, kernel, "ramp", y, 7, length)
                _per_frame(C, orc, s, kernel, "ramp", y, length)
            Fs = FS.special_batches(s)[BATCHES.index(F)]
            _fixed(C, orc, s, kernel, "special", FS.special(s, Fs), 6)
            if s.edit == "literal":
                alphas = (1.0,)  # the host statement is defined on block shifts
            else:
                alphas = (1.0, 0.75)
            for alpha in alphas:
                _fixed(C, orc, s, kernel, "ramp", y, 7, alpha=alpha)
                _per_frame(C, orc, s, kernel, "ramp", y, alpha=alpha)
        if large:
            _per_frame(C, orc, s, kernel, "ramp", FS.ramp(s, 8))
            continue
        for length in (0, N):  # the batch whose frames stop at three and more different iterations, and never
            r = _per_frame(C, orc, s, kernel, "ramp", FS.ramp(s, F_RAMP), length)
            it = r["iters"].cpu().numpy()
            assert it[0] == 1 and (it == MAXIT).any() and np.unique(it).size >= 3
    assert large or any(1 < it < MAXIT for it in stops)


@pytest.mark.parametrize("F", [F for F in FS.BATCH_SIZES if F != 1030])
def test_batch_sizes(C, orc, F):
    """(4, 10, 7): 261 frames are two workgroups in x of the VEC 1 kernels and of k_flags, 1028 two of the VEC 4 kernels with
    four frames in the second."""
    s = FS.by_id("J4_L10_Z7")
    y = FS.ramp(s, F)
    for kernel in _kernels(C, s):
        for its in FS.FIXED_ITS:
            _fixed(C, orc, s, kernel, "ramp", y, its)
        it = _global(C, orc, s, kernel, F)
        assert F == 1 or 1 < it < MAXIT
        r = _per_frame(C, orc, s, kernel, "ramp", y)
        assert F < F_RAMP or np.unique(r["iters"].cpu().numpy()).size >= 3


def test_max_iter_above_64_on_a_table_only_shape(C, orc):
    s = FS.by_id("J3_L9_Z50")
    code = _code(C, s)
    for F in BATCHES:
        y = FS.slow_batch(s, F)
        want = FS.want_global(orc, s, "slow", y, max_iter=70)
        assert want["it"] > 64
        for kernel in _kernels(C, s):
            r = _decode(C, code, y, max_iter=70, exit_mode=C.EXIT_BATCH_GLOBAL, kernel=kernel, want_flag_hist=True)
            _same(code, r, want, "max_iter 70, F=%d kernel=%d" % (F, kernel), 70)
            _ran(C, code, s, kernel, F)


def test_misaligned_input_takes_the_scalar_kernels(C, orc):
    """F = 8 with y one float into a larger buffer: not 16-byte aligned, so the VEC 4 kernels may not load it."""
    for s in (FS.by_id("J4_L10_Z7"), FS.by_id("J3_L26_Z64_wc24")):
        code, F = _code(C, s), 8
        y = FS.ramp(s, F)
        buf = torch.zeros(code.N * F + 4, dtype=torch.float32, device="cuda")
        off = buf[1:1 + code.N * F].view(code.N, F)
        off.copy_(_t(y))
        assert off.is_contiguous() and off.data_ptr() % 16 == 4 and _t(y).data_ptr() % 16 == 0
        for mode, want in ((C.EXIT_FIXED, FS.want_fixed(orc, s, "ramp", y, 7)), (C.EXIT_PER_FRAME, FS.want_per_frame(orc, s, "ramp", y))):
            its = 7 if mode == C.EXIT_FIXED else MAXIT
            a = C.LDPC_Decoder_GPU(code, _t(y), max_iter=its, exit_mode=mode, kernel=C.KERNEL_TABLE, want_app=True)
            assert code.last_kernel == "table_vec4"
            b = C.LDPC_Decoder_GPU(code, off, max_iter=its, exit_mode=mode, kernel=C.KERNEL_TABLE, want_app=True)
            torch.cuda.synchronize()
            assert code.last_kernel == "table_vec1"
            _same(code, b, want, "%s misaligned y, mode %d" % (shape_id(s), mode))
            assert torch.equal(a["D"], b["D"]) and torch.equal(a["app"].view(torch.int32), b["app"].view(torch.int32))
        c = C.LDPC_Decoder_GPU(code, off, max_iter=7, exit_mode=C.EXIT_FIXED, kernel=C.KERNEL_TABLE, alpha=1.0, want_app=True)
        torch.cuda.synchronize()
        assert code.last_kernel == "table_vec1_norm"
        _same(code, c, FS.want_fixed(orc, s, "ramp", y, 7), "%s misaligned y, normalised" % shape_id(s))


def _counters(orc, s, want, length, cw=None):
    """The oracle's Statistic on the oracle's D: the batch at once, or (per-frame exit) frame after frame with its own count."""
    N, F = s.L * s.Z, want["D"].shape[1]
    cnt = np.zeros(5, np.int64)
    length = length or (s.L - s.J) * s.Z
    if "iters" in want:
        for f in range(F):
            orc.bldpc_statistic(cnt, f + 1, np.ascontiguousarray(want["D"][:, f]), N, 1, length, int(want["iters"][f]),
                                codeword=None if cw is None else np.ascontiguousarray(cw[:, f]))
    else:
        orc.bldpc_statistic(cnt, F, np.ascontiguousarray(want["D"]), N, F, length, want["it"], codeword=cw)
    return cnt.tolist()


def _sim_counters(SIM):
    return [SIM.num_Error_Frames, SIM.num_Error_Bits, SIM.Total_Iteration, SIM.num_False_Frames, SIM.num_Alarm_Frames]


@pytest.mark.parametrize("ident,F", [("J3_L5_Z13", 5), ("J3_L5_Z13", 8), ("J4_L10_Z7", 1028), ("J4_L10_Z7", 1030), ("J3_L26_Z64_wc24", 5),
                                     ("J3_L26_Z64_wc24", 8)])
def test_statistics(C, orc, ident, F):
    """bldpc_decode_statistic, and bldpc_decode followed by bldpc_statistic, against the oracle's Statistic on the oracle's D:
    one slice (length below 64), a last slice that is not full (N - 1, and N = 65), F above 1024 as a multiple of 4 and not."""
    s = FS.by_id(ident)
    code, N, K = _code(C, s), s.L * s.Z, (s.L - s.J) * s.Z
    y = FS.ramp(s, F)
    gkey, gy = FS.global_ramp(s, F)
    errors = 0
    for length in (1, 31, 33, K, N - 1, N):
        wants = {C.EXIT_FIXED: (y, FS.want_fixed(orc, s, "ramp", y, 7, length)),
                 C.EXIT_BATCH_GLOBAL: (gy, FS.want_global(orc, s, gkey, gy, length=length)),
                 C.EXIT_PER_FRAME: (y, FS.want_per_frame(orc, s, "ramp", y, MAXIT, length))}
        for mode, (yy, want) in wants.items():
            cnt = _counters(orc, s, want, length)
            errors += cnt[1]
            its = 7 if mode == C.EXIT_FIXED else MAXIT
            for kernel in (C.KERNEL_AUTO, C.KERNEL_TABLE):
                what = "%s F=%d length=%d mode=%d kernel=%d" % (ident, F, length, mode, kernel)
                dev = torch.zeros(5, dtype=torch.int64, device="cuda")
                q = C.Decode_Statistic(code, _t(yy), dev, max_iter=its, length=length, exit_mode=mode, kernel=kernel)
                assert dev.cpu().tolist() == cnt, "Decode_Statistic: %s: %s, not %s" % (what, dev.cpu().tolist(), cnt)
                assert np.array_equal(q["D"].cpu().numpy(), want["D"]), what
                r = C.LDPC_Decoder_GPU(code, _t(yy), max_iter=its, length=length, exit_mode=mode, kernel=kernel)
                SIM = C.SimCounters()
                C.Statistic(SIM, code, r["D"], r["iters"] if mode == C.EXIT_PER_FRAME else r["iteraTime"], length=length)
                assert _sim_counters(SIM) == cnt, "Statistic: %s: %s, not %s" % (what, _sim_counters(SIM), cnt)
    assert errors > 0, "the batches must hold bit errors"
    # a codeword that is not zero: Statistic counts the differences (the decoder still saw the all-zero word's channel)
    cw = (np.random.default_rng(3).random((N, F)) < 0.3).astype(np.int32)
    cwt = torch.from_numpy(cw).cuda()
    for length in (33, N - 1):
        want = FS.want_fixed(orc, s, "ramp", y, 7, length)
        r = C.LDPC_Decoder_GPU(code, _t(y), max_iter=7, length=length, exit_mode=C.EXIT_FIXED)
        SIM = C.SimCounters()
        C.Statistic(SIM, code, r["D"], r["iteraTime"], length=length, CodeWord=cwt)
        assert _sim_counters(SIM) == _counters(orc, s, want, length, cw)


def test_device_refusals(C, orc):
    """KERNEL_QC_LDS on codes the fused kernels do not take: refused as unsupported, in the same words the second time, and the
    table kernels of the same code object decode as before."""
    from cuda_ldpc_amd._lib import LdpcError
    for ident in ("J4_L10_Z7", "J3_L9_Z50_literal", "J6_L129_Z64_wc24", "J63_L64_Z64", "J3_L26_Z64_wc25", "J4_L97_Z96_wc24_wide",
                  "J3_L27_Z1024_wc24"):
        s = FS.by_id(ident)
        code, y = _code(C, s), FS.ramp(s, 8)
        before = _fixed(C, orc, s, C.KERNEL_TABLE, "ramp", y, 7)
        for mode, alpha in ((C.EXIT_FIXED, None), (C.EXIT_PER_FRAME, None), (C.EXIT_BATCH_GLOBAL, None), (C.EXIT_FIXED, 0.75)):
            said = []
            for _ in range(2):
                with pytest.raises(LdpcError, match=r"\(-5\): .*QC_LDS kernel unavailable") as e:
                    C.LDPC_Decoder_GPU(code, _t(y), max_iter=7, exit_mode=mode, kernel=C.KERNEL_QC_LDS, alpha=alpha)
                said.append(str(e.value))
            assert said[0] == said[1]
        after = _fixed(C, orc, s, C.KERNEL_TABLE, "ramp", y, 7)
        assert torch.equal(before["D"], after["D"]) and torch.equal(before["app"].view(torch.int32), after["app"].view(torch.int32))


def test_one_code_object_through_shrinking_and_growing_batches(C, orc):
    """A code object of its own, whose scratch is sized by the largest call: 1028 frames, then 1, then 1028 again."""
    s = FS.by_id("J4_L10_Z7")
    fresh = FS.make_code(C, s)
    seen = []
    for F in (1028, 1, 1028):
        y = FS.ramp(s, F)
        a = _fixed(C, orc, s, C.KERNEL_AUTO, "ramp", y, 7, code=fresh)
        b = _per_frame(C, orc, s, C.KERNEL_TABLE, "ramp", y, code=fresh)
        _global(C, orc, s, C.KERNEL_AUTO, F, code=fresh)
        seen.append((a["D"].clone(), a["app"].clone(), b["D"].clone(), b["iters"].clone()))
    assert all(torch.equal(p, q) for p, q in zip(seen[0], seen[2]))
    fresh.close()
