"""What tests/test_qc_variants_gpu.py relies on, checked without a GPU: every entry of the fused kernels' variant table has a
case, every case's matrix fits the entry it is meant for, and the oracle alone confirms that the chosen Es/N0 and seeds exercise
what the GPU tests say they exercise (a batch-global stop strictly inside (1, max_iter), frames that stop at different iterations,
the wrap counts of the seeded shift sets, the pass orders of the ran_to_max test)."""
import numpy as np
import pytest

import qc_variant_cases as Q


@pytest.fixture(scope="module")
def C():
    import cuda_ldpc_amd
    return cuda_ldpc_amd


@pytest.fixture(scope="module")
def variants(C):
    return C.qc_variants()


@pytest.fixture(scope="module")
def cases(variants):
    return Q.build_cases(variants)


def test_variant_table_is_readable_without_a_device(C, variants):
    import ctypes
    from cuda_ldpc_amd._lib import lib
    assert len(variants) == lib.bldpc_qc_variant_count() >= 29
    info = np.zeros(16, np.int32)
    for bad in (-1, len(variants)):
        assert lib.bldpc_qc_variant_info(bad, info.ctypes.data_as(ctypes.c_void_p), None) != 0
    assert lib.bldpc_qc_variant_info(0, info.ctypes.data_as(ctypes.c_void_p), None) == 0  # the tag is optional
    assert lib.bldpc_code_qc_info(None, info.ctypes.data_as(ctypes.c_void_p)) != 0
    tags = {"row", "row-local", "halfrow", "halfrow-local", "compressed", "regstate", "regstate-halo"}
    for v in variants:
        assert v["tag"] in tags and v["NF"] in (1, 2) and v["Z"] % 32 == 0 and v["threads"] % 64 == 0 and 0 < v["threads"] <= 1024
        assert (v["tag"] == "compressed") == (v["U"] > 0) and (v["regstate"] > 0) == v["tag"].startswith("regstate")
        assert (v["loc"] > 0) == v["tag"].endswith("-local")
        assert v["has_pf"] == (v["loc"] != 2)  # only the row kernel with local edges hands the per-frame exit to another entry
        assert v["lds_bytes"] <= 160 * 1024


def test_every_variant_has_a_case(variants, cases):
    """Adding a table entry without a case fails here."""
    assert sorted(set(c.variant for c in cases)) == list(range(len(variants)))
    assert len(set(c.id for c in cases)) == len(cases)
    for c in cases:
        assert set(c.env) <= {"BLDPC_QC_VARIANT", "BLDPC_NO_LOCAL", "BLDPC_NO_HALO"}
        assert c.env.get("BLDPC_QC_VARIANT", str(c.variant)) == str(c.variant)


def _accepts(v, H, J, L, Z, env):
    """The conditions under which qc_plan_build lets entry v take the matrix, restated (the matching of the local-edge entries
    is not: the GPU test asserts the index the plan reports)."""
    wr, wc = (H >= 0).sum(1), (H >= 0).sum(0)
    Wc, Wcmin, Wv = int(wr.max()), int(wr.min()), int(wc.max())
    if v["Z"] != Z or v["WC"] < Wc:
        return False
    if v["regstate"]:
        if v["regstate"] == 2:
            worst = Q.max_wrapped(H, Z)
            if "BLDPC_NO_HALO" in env or worst is None or worst > v["CPT"]:
                return False
        lds = L * (Z + 64) * 4 + 272 if v["regstate"] == 2 else L * Z * 4 + 16
        return (v["J"], v["L"]) == (J, L) and v["MINW"] <= Wcmin and lds <= 160 * 1024 and bool((wc == J).any()) and bool((wc > 0).all())
    if v["U"]:
        lds = (J + 1) * Z * 12 + (L + 1) * Z * 4 + 16
        return -(-L // v["G"]) <= v["CPT"] and Wv <= 28 and J <= 62 and L <= 254 and lds <= 160 * 1024
    if (v["J"], v["L"]) != (J, L) or v["WV"] < Wv:
        return False
    if v["loc"] and "BLDPC_NO_LOCAL" in env:
        return False
    if v["loc"] == 1:
        return Wcmin == v["WC"] and L % (2 * J) == 0
    if v["loc"] == 2:
        return Z % 64 == 0 and int(wc.min()) == v["WV"] and Wcmin >= L // J
    return True


def _plan_host(C, c):
    """qc_plan_host for the case's matrix under the case's pin and switches."""
    return C.qc_plan_host(Q.matrix(c.matrix)[1], Q.matrix(c.matrix)[4], pin=int(c.env.get("BLDPC_QC_VARIANT", -1)),
                          no_local="BLDPC_NO_LOCAL" in c.env, no_halo="BLDPC_NO_HALO" in c.env)


def test_every_case_fits_its_variant(C, variants, cases):
    for c in cases:
        _, H, J, L, Z = Q.matrix(c.matrix)
        v = variants[c.variant]
        assert _accepts(v, H, J, L, Z, c.env), (c.id, v)
        assert _plan_host(C, c).variant == c.variant, c.id  # the real selection, the local-edge matching included
        if v["tag"] == "compressed":
            assert -(-L // v["G"]) <= v["CPT"], c.id  # the CPT bound
        earlier = [u["index"] for u in variants[:c.variant] if _accepts(u, H, J, L, Z, c.env)]
        if "BLDPC_QC_VARIANT" in c.env:
            assert earlier, "%s is pinned, but nothing stands in front of variant %d: use the product path" % (c.id, c.variant)
        else:
            assert not earlier, "%s: variants %s take the matrix before %d" % (c.id, earlier, c.variant)


def _fnv1a(data):
    h = 1469598103934665603
    for x in data:
        h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_plan_tables_equal_the_parent_commit(C, cases):
    """tests/golden/qc_plan_digests.json holds, per case, what qc_plan_build handed to the device BEFORE it was split into stages (its
    hipMalloc / hipMemcpy redirected to host stand-ins, the bytes behind the plan's pointers hashed): the table entry, the LDS
    size and every table of the staged build are those, byte for byte."""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qc_plan_digests.json")) as f:
        want = json.load(f)
    assert sorted(want) == sorted(c.id for c in cases)
    for c in cases:
        w = want[c.id]
        H = np.ascontiguousarray(Q.matrix(c.matrix)[1], np.int32)
        assert "%016x" % _fnv1a(H.tobytes()) == w["h"], "%s: numpy has generated another matrix than the fixture was made from" % c.id
        got = _plan_host(C, c)
        assert got.info.tolist() == w["info"], c.id
        assert ["%016x" % int(x) for x in got.digest] == w["digest"], c.id


def test_plan_host_refuses_bad_arguments(C):
    H = Q.matrix(("shipped", "J4_L24_Z96"))[1]
    with pytest.raises(C._lib.LdpcError):
        C.qc_plan_host(H, 0)
    with pytest.raises(C._lib.LdpcError):
        C.qc_plan_host(H, 64)  # shifts of a Z = 96 matrix
    none = C.qc_plan_host(H, 96, pin=10 ** 6)  # a pin that names no entry: no plan, not an error
    assert none.info.tolist() == [-1, -1, 0, 0, 0, 0, 0, 0] and not none.digest.any()


def test_reachable_by_pin_only(variants, cases):
    """The entries DESIGN.md lists as reachable by pin only are those whose every accepted matrix an earlier entry accepts:
    here, the entries none of whose cases runs without a pin."""
    unpinned = set(c.variant for c in cases if "BLDPC_QC_VARIANT" not in c.env)
    pin_only = [v for v in variants if v["index"] not in unpinned]
    assert sorted((v["tag"], v["J"], v["Z"]) for v in pin_only) == [("row", 4, 96), ("row", 6, 96), ("row", 8, 96), ("row", 12, 96)]


def test_seeded_shift_sets_need_the_variant_they_are_meant_for(variants, cases):
    by_id = {c.id: c for c in cases}
    _, H, _, _, Z = Q.matrix(by_id["regstate-Z512-shifts"].matrix)
    halo = variants[Q.find_variant(variants, "regstate-halo", J=4, Z=512)]
    assert Q.max_wrapped(H, Z) > halo["CPT"] == 5  # more wrapped blocks in one (row, tile) than the halo entry has slots
    assert Q.max_wrapped(Q.matrix(("shipped", "J4_L24_Z512"))[1], Z) <= halo["CPT"]
    _, H, _, _, Z = Q.matrix(by_id["halo-J15-ng3-shifts"].matrix)
    assert Q.max_wrapped(H, Z) == 3 == variants[by_id["halo-J15-ng3-shifts"].variant]["CPT"]
    assert Q.max_wrapped(Q.matrix(("shipped", "J15_L30_Z1280"))[1], Z) <= 2


def test_oracle_conditions_of_every_case(orc, cases):
    for spec, snr in sorted(set((c.matrix, c.snr) for c in cases)):
        w = Q.want_global(orc, spec, snr)
        assert 1 < w["it"] < Q.MAXIT_GLOBAL, "%s at %.1f dB: the batch stops at %d" % (spec, snr, w["it"])
        it = Q.want_per_frame(orc, spec, snr)[2]
        assert len(set(it.tolist())) > 1, "%s at %.1f dB: every frame stops at %s" % (spec, snr, it)
        assert it.min() >= 1 and it.max() <= w["it"]


@pytest.mark.parametrize("name,Fs", [("J4_L24_Z96", (6,)), ("J32_L64_Z64", (5, 6))])
def test_oracle_conditions_of_the_switch_tests(orc, name, Fs):
    spec = ("shipped", name)
    oc = Q.ocode(orc, spec)
    for F in Fs:
        y = Q.channel(orc, spec, Q.SNR[spec], F)
        w = orc.bldpc_decode(oc, y, F, Q.MAXIT_GLOBAL, early_exit=1)
        assert 1 < w["it"] < Q.MAXIT_GLOBAL
        assert len(set(Q.oracle_per_frame(orc, oc, y, F, Q.MAXIT_GLOBAL)[2].tolist())) > 1


@pytest.mark.parametrize("name", ["J4_L24_Z96", "J8_L24_Z96"])
def test_oracle_conditions_of_the_ran_to_max_test(orc, name):
    """`never` runs to max_iter with a frame unflagged (the hint is set whichever pass came first); `early` stops inside, at the
    latest first flag of its frames: stop == run after a per-frame pass, stop < run = max_iter after a full run."""
    spec = ("shipped", name)
    _, _, _, L, Z = Q.matrix(spec)
    N, F, maxit = L * Z, Q.F_EXIT, Q.MAXIT_GLOBAL
    oc = Q.ocode(orc, spec)
    y_early, y_never = Q.channel(orc, spec, Q.SNR[spec], F), Q.channel(orc, spec, Q.SNR[spec] - 6.0, F)
    w_never = orc.bldpc_decode(oc, y_never, F, maxit, early_exit=1)
    assert w_never["it"] == maxit and not np.all(w_never["D"].reshape(N + 1, F)[N] == 1)
    w_early = orc.bldpc_decode(oc, y_early, F, maxit, early_exit=1)
    assert 1 < w_early["it"] < maxit
    assert int(Q.oracle_per_frame(orc, oc, y_early, F, maxit)[2].max()) == w_early["it"]
