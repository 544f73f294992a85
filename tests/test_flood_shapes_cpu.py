"""The references and the inputs of tests/test_flood_shapes_gpu.py, without a GPU, on the shape table of tests/flood_shape_cases.py:
the generator and its post-edits keep their promises; the CPU oracle and the numpy restatement of test_binary_crosscheck_cpu.py
agree bit for bit on every shape (the as-written table against a restatement over the address table, written here);
bldpc_decode_normalised_host equals the oracle at alpha 1 and the numpy restatement of test_normalised_cpu.py at alpha 0.75; the
ramp input makes frames stop at different iterations and never, and the recorded sub-batches stop under the batch-global rule
strictly inside (1, MAXIT); bldpc_qc_plan_host routes every shape where the table says; the refusals that need no device."""
import numpy as np
import pytest

import flood_shape_cases as FS
from flood_shape_cases import BATCHES, F_RAMP, GRID_CAP, LARGE, MAXIT, SHAPES, shape_id
from test_binary_crosscheck_cpu import np_minsum
from test_layered_shapes_cpu import random_blockh
from test_normalised_cpu import np_norm_minsum, same_bits

EXIT_FIXED, EXIT_PER_FRAME = 0, 2
QC = [s for s in SHAPES if s.edit != "literal"]  # the shapes made from block shifts


@pytest.fixture(scope="module")
def C():
    import cuda_ldpc_amd
    return cuda_ldpc_amd


def test_generator_and_edits_keep_their_promises():
    assert len({shape_id(s) for s in SHAPES}) == len(SHAPES)
    for s in SHAPES:
        H = FS.matrix_of(s)
        nz = H != -1
        wc, wv = nz.sum(1), nz.sum(0)
        assert H.shape == (s.J, s.L) and H.dtype == np.int32 and H.min() >= -1 and H.max() < s.Z, shape_id(s)
        assert wc.min() >= 2 and wc.max() <= 26 and wv.max() <= 16, shape_id(s)
        if s.weights is not None and s.edit != "empty":
            assert tuple(wc) == tuple(s.weights), shape_id(s)
        assert (wv.min() == 0) == (s.edit in ("empty", "wide")), shape_id(s)
        if s.edit in ("empty", "wide"):
            assert (wv == 0).sum() == 1
        flat = H.reshape(-1)[nz.reshape(-1)]
        assert flat[0] == 0 and flat[-1] == s.Z - 1, shape_id(s)
        assert np.array_equal(H, FS.generate(s)), "deterministic in the table"
        if s.edit is None:
            assert np.array_equal(H, random_blockh(s.J, s.L, s.Z, s.J + s.L + s.Z, s.weights))
    H = FS.matrix_of(FS.by_id("J17_L40_Z33_wc26_wv16"))
    nz = H != -1
    assert nz[:16, FS.WV16_COL].all() and not nz[16, FS.WV16_COL] and nz.sum(0)[FS.WV16_COL] == 16
    assert nz.sum(0)[FS.WV1_COL] == 1 and {2, 26} <= set(nz.sum(1).tolist())
    H = FS.matrix_of(FS.by_id("J6_L121_Z64_wc24_twin"))
    a, b = np.flatnonzero(H[1] != -1)[:2]
    assert H[1, a] == H[1, b]
    assert (FS.matrix_of(FS.by_id("J4_L96_Z96_wc24")) != -1).sum(0).tolist() == [1] * 96
    assert np.array_equal(FS.matrix_of(FS.by_id("J3_L9_Z50_literal")), FS.matrix_of(FS.by_id("J3_L9_Z50")))
    s = FS.by_id("J32_L33_Z2053")
    assert s[:3] == LARGE and s.J * s.Z > GRID_CAP and s.L * s.Z > GRID_CAP
    y = FS.ramp(s, 5)
    assert y.dtype == np.float32 and (y[:, 0] == 1.0).all() and not y.flags.writeable


def np_table_minsum(addr, Z, wc, wv, y, iters):
    """Flooding min-sum over an address table [N, Wv] (any table, colliding slots included), one variable node after the other in
    ascending order as the reference's kernel is defined on one frame: S = ((0 + R_0) + R_1 ...) + y, every slot then takes S - R;
    the check rows as np_minsum has them.  Returns (D, S)."""
    N, F = y.shape
    J, Wc = len(wc) - 1, int(wc[-1])
    rq = np.zeros((J * Z * Wc, F), np.float32)
    S_all = np.zeros((N, F), np.float32)
    for it in range(iters):
        for n in range(N):
            ad = addr[n, :wv[n // Z]]
            R = rq[ad]
            S = np.zeros(F, np.float32)
            for r in R:
                S = S + r
            S = S + y[n]
            S_all[n] = S
            for a, r in zip(ad, R):
                rq[a] = S - r
        for m in range(J * Z):
            w = int(wc[m // Z])
            Q = rq[m * Wc:m * Wc + w]
            sg = np.where(Q < 0, -1, 1).astype(np.int32)
            a = np.where(Q < 0, -Q, Q)
            P = np.prod(sg, axis=0)
            srt = np.sort(a, axis=0)
            idx = np.argmax(a == srt[0][None], axis=0)
            for i in range(w):
                rq[m * Wc + i] = (P * sg[i]).astype(np.float32) * np.where(idx == i, srt[1], srt[0])
    return (S_all < 0).astype(np.int32), S_all


@pytest.mark.parametrize("s", SHAPES, ids=shape_id)
def test_oracle_equals_numpy_restatement(C, orc, s):
    F = 2 if s[:3] == LARGE else 5
    y = FS.ramp(s, F)
    H = FS.matrix_of(s)
    oc = FS.ocode(orc, s)
    assert oc.N == s.L * s.Z and np.array_equal(oc.H.reshape(s.J, s.L), H)
    if s.edit == "literal":
        wc, wv = FS.row_col_weights(H)
        addr = C.Transform_H(H, s.J, s.L, s.Z, wc, wv, as_written=True)
        assert np.array_equal(addr, oc.addr) and np.array_equal(wc, oc.wc) and np.array_equal(wv, oc.wv)
        edges = int(wv[:-1].sum()) * s.Z
        assert len(np.unique(addr[addr >= 0])) < edges, "the as-written table must make slots collide"
    for its in FS.FIXED_ITS:
        want = FS.want_fixed(orc, s, "ramp", y, its)
        if s.edit == "literal":
            D, S = np_table_minsum(addr.reshape(oc.N, -1), s.Z, wc, wv, y, its)
        else:
            D, S = np_minsum(H, s.Z, y, its)
        assert np.array_equal(D, want["D"][:oc.N]), "hard bits, %d iterations" % its
        assert same_bits(S, want["app"]), "a-posteriori bits, %d iterations" % its


@pytest.mark.parametrize("s", QC, ids=shape_id)
def test_normalised_host_on_the_shapes(C, orc, s):
    large = s[:3] == LARGE
    F = 2 if large else 5
    y = FS.ramp(s, F)
    H, N = FS.matrix_of(s), s.L * s.Z
    host = lambda yy, its, alpha, **kw: C.normalised_host(H, s.J, s.L, s.Z, yy, max_iter=its, alpha=alpha, **kw)
    for its in FS.FIXED_ITS:
        want = FS.want_fixed(orc, s, "ramp", y, its)
        got = host(y, its, 1.0)
        assert np.array_equal(got["D"], want["D"]) and same_bits(got["app"], want["app"]), "alpha 1, %d iterations" % its
        D, S = np_norm_minsum(H, s.Z, y, its, 0.75)
        got = host(y, its, 0.75)
        assert np.array_equal(got["D"], D) and same_bits(got["app"], S), "alpha 0.75, %d iterations" % its
        assert (got["iters"] == its).all()
    if large:
        return
    want = FS.want_per_frame(orc, s, "ramp", y)
    got = host(y, MAXIT, 1.0, exit_mode=EXIT_PER_FRAME)
    assert np.array_equal(got["iters"], want["iters"]) and np.array_equal(got["D"], want["D"]) and same_bits(got["app"], want["app"])
    # alpha 0.75 under per-frame exit: every frame is the fixed-iteration run of its own count, whose flag was down one iteration earlier
    for length in (0, N):
        got = host(y, MAXIT, 0.75, exit_mode=EXIT_PER_FRAME, length=length)
        for f in range(F):
            it, yf = int(got["iters"][f]), np.ascontiguousarray(y[:, f:f + 1])
            one = host(yf, it, 0.75, length=length)
            assert np.array_equal(one["D"][:, 0], got["D"][:, f]) and same_bits(one["app"][:, 0], got["app"][:, f]), "frame %d" % f
            assert got["D"][N, f] == 1 or it == MAXIT
            assert it == 1 or host(yf, it - 1, 0.75, length=length)["D"][N, 0] == 0


@pytest.mark.parametrize("s", SHAPES, ids=shape_id)
def test_the_ramp_stops_frames_where_the_gpu_tests_need_it(orc, s):
    """Judged by the oracle alone, prefix rule, MAXIT iterations, length 0 (K) and N."""
    N = s.L * s.Z
    large = s[:3] == LARGE
    batches = (8,) if large else (F_RAMP,) + tuple(F for F in FS.BATCH_SIZES if F >= F_RAMP and s[:3] == (4, 10, 7))
    for F in batches:
        for length in (0, N):
            it = FS.want_per_frame(orc, s, "ramp", FS.ramp(s, F), length=length)["iters"]
            what = "%s F=%d length=%d: iters %s" % (shape_id(s), F, length, it.tolist())
            assert it[0] == 1 and ((it > 1) & (it < MAXIT)).any() and (it == MAXIT).any(), what
            assert F < F_RAMP or np.unique(it).size >= 3, what
    if large:
        return
    widths = {F: FS.global_width(s, F) for F in (tuple(FS.BATCH_SIZES) if s[:3] == (4, 10, 7) else ()) + BATCHES}
    assert any(widths.values()), shape_id(s)
    for F, W in widths.items():
        key, y = FS.global_ramp(s, F)
        assert y.shape == (N, F) and key == ("ramp", W or F)
        for length in (0, N):
            it = FS.want_global(orc, s, key, y, length=length)["it"]
            if W:
                assert 1 < it < MAXIT, "%s F=%d W=%d length=%d stops at %d" % (shape_id(s), F, W, length, it)


def test_the_special_values_keep_the_sums_finite(orc):
    """+-3e38 must not meet through a block row of weight 2 (see SPECIAL_BATCHES): every batch the GPU test uses keeps the oracle's
    sums finite in all 6 iterations, and the one batch that is left out does overflow."""
    for s in SHAPES:
        for F in FS.special_batches(s):
            y = FS.special(s, F)
            assert np.isfinite(y).all() and y.shape == (s.L * s.Z, F)
            for its in range(1, 7):
                assert np.isfinite(FS.want_fixed(orc, s, "special", y, its)["app"]).all(), "%s F=%d, %d iterations" % (shape_id(s), F, its)
    assert set(FS.SPECIAL_BATCHES) == {(3, 8, 2048)}
    s = FS.by_id("J3_L8_Z2048")
    assert (FS.matrix_of(s) != -1).sum(1).min() == 2
    app = FS.want_fixed(orc, s, "special", FS.special(s, 5), 2)["app"]
    assert np.isinf(app).sum() == 2 and np.isnan(FS.want_fixed(orc, s, "special", FS.special(s, 5), 4)["app"]).any()


def test_the_slow_batch_runs_past_64_iterations(orc):
    s = FS.by_id("J3_L9_Z50")
    for F in BATCHES:
        assert FS.want_global(orc, s, "slow", FS.slow_batch(s, F), max_iter=70)["it"] == 70


def test_routing(C):
    """bldpc_qc_plan_host sends every shape where the table says: the compressed entry of its Z up to L = CPT * G, J = 62, row
    weight WCS and the LDS bound, the table kernels one past each of them and wherever Z has no entry."""
    variants = C.qc_variants()
    tags = {}
    for s in QC:
        p = C.qc_plan_host(FS.matrix_of(s), s.Z)
        tags[shape_id(s)] = None if p.variant < 0 else variants[p.variant]["tag"]
        assert tags[shape_id(s)] == s.landing, shape_id(s)
        if s.landing:
            v = variants[p.variant]
            assert v["Z"] == s.Z and p.variant_per_frame == -1
            assert (s.L + v["G"] - 1) // v["G"] <= v["CPT"] and s.J <= 62 and (FS.matrix_of(s) != -1).sum(1).max() <= v["WC"]
            assert p.lds_bytes == 12 * (s.J + 1) * s.Z + 4 * (s.L + 1) * s.Z + 16 <= 160 * 1024
    entry = lambda Z: next(v for v in variants if v["tag"] == "compressed" and v["Z"] == Z)
    v64, v96, v1024 = entry(64), entry(96), entry(1024)
    assert (v64["G"], v64["CPT"], v64["WC"]) == (16, 8, 24) and (v96["U"], v96["G"], v96["CPT"]) == (128, 8, 12)
    assert 12 * 4 * 1024 + 4 * 27 * 1024 + 16 == 159760 and 12 * 4 * 1024 + 4 * 28 * 1024 + 16 == 160 * 1024 + 16
    assert v1024["G"] * v1024["CPT"] >= 27, "(3, 27, 1024) must fail on LDS alone"
    for Z in (1, 7, 13, 33, 50, 500, 32, 2048, 2053):
        assert not [v for v in variants if v["Z"] == Z], Z
    pairs = [("J6_L128_Z64_wc24", "J6_L129_Z64_wc24"), ("J62_L64_Z64", "J63_L64_Z64"), ("J3_L26_Z64_wc24", "J3_L26_Z64_wc25"),
             ("J4_L96_Z96_wc24", "J4_L97_Z96_wc24_wide"), ("J3_L26_Z1024_wc24", "J3_L27_Z1024_wc24")]
    for inside, past in pairs:
        assert tags[inside] == "compressed" and tags[past] is None, (inside, past)


def test_refusals_that_need_no_device(C):
    """bldpc_code_create_qc refuses a block column of weight 17, a block row of weight 27 and J >= L before it touches a device,
    in the same words the second time."""
    from cuda_ldpc_amd._lib import LdpcError
    col17 = random_blockh(18, 40, 33, 1, (12,) * 18)
    col17[:17, 3], col17[17, 3] = 1, -1
    wv = (col17 != -1).sum(0)
    assert wv[3] == 17 and np.delete(wv, 3).max() <= 16 and (col17 != -1).sum(1).max() <= 13
    row27 = random_blockh(3, 28, 64, 21, (27, 5, 5))
    square = random_blockh(4, 5, 7, 3)[:, :4]
    for H, Z, pattern in ((col17, 33, r"\(-5\): .*Wv=17"), (row27, 64, r"\(-5\): .*Wc=27"), (square, 7, r"J < L")):
        said = []
        for _ in range(2):
            with pytest.raises(LdpcError, match=pattern) as e:
                C.BinaryCode.from_shifts(H, H.shape[0], H.shape[1], Z)
            said.append(str(e.value))
        assert said[0] == said[1] and said[0].strip()
