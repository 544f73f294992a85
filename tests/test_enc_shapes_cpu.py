"""The generated encoder cases of tests/enc_shape_cases.py without a GPU: every case has the property it is there for (judged by the
numpy reference alone), both host generators equal the reference bit for bit, the GF(q) message rule holds at m = 2, 3, 5, 7, and
the host generators run as a stand-alone program (tests/cpp/encoder_host_test.hip) under the address + undefined and the thread
sanitizer on every case and on the two shipped matrices large enough for the threaded passes to spawn threads.
tests/test_enc_shapes_gpu.py holds the device kernels against the same reference."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import enc_shape_cases as E
import nb_shape_cases as S
from conftest import DATA


@pytest.fixture(scope="module")
def C():
    import cuda_ldpc_amd
    return cuda_ldpc_amd


@pytest.fixture(scope="module")
def nb():
    from cuda_ldpc_amd import nbldpc
    return nbldpc


# ---- the cases are what the table says ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", E.B_IDS)
def test_binary_case_has_its_property(cid):
    c = E.B_BY_ID[cid]
    H = E.bin_h(cid)
    ref = E.bin_ref(cid)
    N, M, K, rank, pos = c.L * c.Z, c.J * c.Z, ref["K_info"], ref["rank"], ref["info_pos"]
    assert H.shape == (c.J, c.L) and (H >= -1).all() and (H < c.Z).all()
    assert ((H >= 0).sum(0) >= 1).all(), "every block column keeps a block"
    assert ((H >= 0).sum(1) >= 2).all() and ((H >= 0).sum(1) <= 26).all(), "a code object takes 2 ... 26 blocks per block row"
    assert K + rank == N and rank <= M and np.all(np.diff(pos) > 0)
    if cid != "lds_over":
        assert np.array_equal(E.block_matrix(c.J, c.L, c.Z, c.seed, c.density, c.dup), H), "deterministic in the seed"
        assert not np.array_equal(E.block_matrix(c.J, c.L, c.Z, c.seed + 100, c.density, c.dup), H), "another seed is another matrix"
    KW = (K + 63) // 64
    if cid == "tiny":
        assert N == 16 and 0 < K < 16
    elif cid == "k_lt_64":
        assert N == 65 and 0 < K < 64 and rank < 64 and M == 39
    elif cid == "n_500":
        assert N % 64 != 0 and K % 64 not in (0, 1) and not np.array_equal(pos, np.arange(K))
    elif cid == "kw_33":
        assert KW == 33
    elif cid == "kw_34_odd":
        assert KW == 34 and rank % 4 != 0 and N % 64 != 0 and c.Z % 2 == 1
    elif cid == "dup_row":
        assert np.array_equal(H[-1], H[0]) and rank <= M - c.Z
    elif cid == "lds_full":
        assert K == E.LDS_MAX_INFO_BITS == 20480
    elif cid == "lds_over":
        assert K > E.LDS_MAX_INFO_BITS and c.L == E.B_BY_ID["lds_full"].L + 1
        assert np.array_equal(H[:, :-1], E.bin_h("lds_full")), "lds_full and one block column more"
    else:
        raise AssertionError("case without a stated property")


def test_shortening_cases_have_scattered_information_positions():
    """k_enc_pack_short indexes rm_map[info_pos[k]]: on these two codes info_pos is not 0 ... K'-1, on both sides of message index 64."""
    for cid in ("n_500", "kw_34_odd"):
        pos = E.bin_ref(cid)["info_pos"]
        assert len(pos) > 65 and not np.array_equal(pos, np.arange(len(pos))), cid


@pytest.mark.parametrize("cid", E.NB_IDS)
def test_nb_case_has_its_property(cid):
    c = E.nb_code(cid)
    ref = E.nb_ref(cid)
    K, rank = ref["K_info"], ref["rank"]
    assert K + rank == c.N and rank <= c.M and 1 <= K
    colw = np.bincount([v for _, v, _ in c.edges], minlength=c.N)
    roww = np.bincount([r for r, _, _ in c.edges], minlength=c.M)
    assert colw.max() <= c.dv and roww.max() <= c.dc and roww.min() >= 1
    assert all(0 < h < c.q and 0 <= r < c.M and 0 <= v < c.N for r, v, h in c.edges)
    if cid in E.NEW:
        q, N, dv, dc, drop, seed = E.NEW[cid]
        assert (K, rank) == E.NEW_WANT[cid]
        assert S.random_graph(N, dv, dc, drop, q, seed) == (c.M, list(c.edges)), "deterministic in the seed"
        Kp, RG = (K + 3) // 4 * 4, (rank + 7) // 8
        if cid == "q8_chunk4":
            assert Kp == K and K % 256 == 4
        elif cid == "q4_pad":
            assert Kp == 556 and (Kp + 255) // 256 == 3 and rank % 8 == 6
        elif cid == "q128_rank1":
            assert rank % 8 == 1 and RG == 17 and RG % 4 == 1
    elif cid.endswith(E.TWIN):
        base = cid[:-len(E.TWIN)]
        b, bref = E.nb_code(base), E.nb_ref(base)
        mul = S.gf_tables(c.q)[0]
        A, A0 = E.dense_hq(c.N, c.M, c.edges), E.dense_hq(b.N, b.M, b.edges)
        a = E.twin_factor(c.q, S.BY_ID[base].seed)
        assert 2 <= a < c.q and np.array_equal(A[:-1], A0[:-1]) and np.array_equal(A[-1], mul[a, A0[0]]) and A[-1].any()
        assert rank < c.M, "rank deficient"
        if bref["rank"] == b.M:
            assert rank == b.M - 1 and K == bref["K_info"] + 1, "the rank drops by 1"
    else:
        assert (c.M, list(c.edges)) == S.graph(S.BY_ID[cid])


def test_nb_fields_and_chunks_the_cases_are_there_for():
    qs = {E.nb_code(cid).q for cid in E.NB_IDS}
    assert {4, 8, 16, 32, 64, 128, 256} <= qs
    assert any(E.nb_ref(cid)["K_info"] > 256 for cid in E.NB_IDS) and any(E.nb_ref(cid)["K_info"] % 4 for cid in E.NB_IDS)
    assert {E.nb_ref(cid)["rank"] % 8 for cid in E.NB_IDS} >= {1, 7}


# ---- the host generators equal the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", E.B_IDS)
def test_binary_generator_host_equals_the_reference(C, cid):
    c = E.B_BY_ID[cid]
    ref = E.bin_ref(cid)
    gen = C.generator_host(E.bin_h(cid), c.J, c.L, c.Z)
    assert (gen["K_info"], gen["rank"]) == (ref["K_info"], ref["rank"])
    assert np.array_equal(gen["info_pos"], ref["info_pos"])
    assert gen["P"].shape == ref["P"].shape and np.array_equal(gen["P"], ref["P"]), "P differs (the pad bits past K' are zero in the reference)"
    K = gen["K_info"]
    if K % 64:
        assert not (gen["P"][:, -1] >> np.uint64(K % 64)).any(), "pad bits of P past K'"
    again = C.generator_host(E.bin_h(cid), c.J, c.L, c.Z)
    assert np.array_equal(again["info_pos"], gen["info_pos"]) and np.array_equal(again["P"], gen["P"])


@pytest.mark.parametrize("cid", E.NB_IDS)
def test_nb_generator_host_equals_the_reference(nb, cid):
    mpath, gpath = E.nb_files(cid)
    c = E.nb_code(cid)
    H = nb.NBMatrix(mpath)
    assert (H.N, H.M, H.q, H.dc) == (c.N, c.M, c.q, c.dc)
    mul, _, _ = nb.GFInitial(c.q, gpath)
    assert np.array_equal(mul, S.gf_tables(c.q)[0])
    ref = E.nb_ref(cid)
    gen = nb.generator_host(H, mul)
    assert (gen["K_info"], gen["rank"]) == (ref["K_info"], ref["rank"])
    assert np.array_equal(gen["info_pos"], ref["info_pos"])
    assert gen["P"].shape == ref["P"].shape and np.array_equal(gen["P"], ref["P"])
    again = nb.generator_host(H, mul)
    assert np.array_equal(again["info_pos"], gen["info_pos"]) and np.array_equal(again["P"], gen["P"])


# ---- the message rule where m does not divide 64 --------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [4, 8, 32, 128])
def test_nb_message_rule_with_python_integers(nb, q):
    from cuda_ldpc_amd.bldpc import splitmix64
    m = q.bit_length() - 1
    s = 64 // m
    seed, first, B = 0xFEDCBA9876543210, 5, 4
    for K in (2 * s + 1, 555):  # three words; and a last word that is not full for any of the four m
        W = -(-K // s)
        got = nb.pn_messages(seed, K, q, B, first_frame=first)
        assert got.shape == (B, K) and got.min() >= 0 and got.max() < q
        for b in range(B):
            for k in (0, s - 1, s, K - 1):
                w = int(splitmix64((seed + (first + b) * W + k // s) % (1 << 64)))
                assert got[b, k] == (w >> (m * (k % s))) & (q - 1), (q, K, b, k)
        assert K < 555 or len(np.unique(got)) == q, "4 x 555 draws hold every element of the field"


# ---- the host generators under the host sanitizers, stand-alone -----------------------------------------------------------------------
SANITIZERS = {"asan_ubsan": ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"],
              "tsan": ["-Xarch_host", "-fsanitize=thread"]}


@pytest.fixture(scope="module", params=list(SANITIZERS))
def gen_exe(request, tmp_path_factory):
    """tests/cpp/encoder_host_test.hip, built as test_nb_shapes_cpu.py builds nb_plan_host_test.hip, once per sanitizer set."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    here = os.path.dirname(os.path.abspath(__file__))
    tmp = tmp_path_factory.mktemp("enc_host_" + request.param)
    exe = str(tmp / "encoder_host")
    subprocess.check_call([hipcc, "-O1", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off"] + SANITIZERS[request.param]
                          + [os.path.join(here, "cpp", "encoder_host_test.hip"), "-o", exe], cwd=str(tmp))
    return exe


def _run(exe, args, gen, timeout):
    r = subprocess.run([exe] + [str(a) for a in args], timeout=timeout, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode()
    assert r.returncode == 0, out  # a sanitizer report ends the program with a nonzero status
    assert "Sanitizer" not in out and "runtime error" not in out, out
    tok = out.strip().split("\n")[-1].split()
    assert (int(tok[0]), int(tok[1])) == (gen["K_info"], gen["rank"]), out
    assert int(tok[2], 16) == E.digest(gen["info_pos"], gen["P"]), "info_pos or P differ from what generator_host returned in Python"
    return int(tok[3])


@pytest.mark.parametrize("cid", E.B_IDS)
def test_binary_generator_stand_alone(C, gen_exe, cid):
    c = E.B_BY_ID[cid]
    _run(gen_exe, ["b", E.bin_file(cid), c.J, c.L, c.Z], C.generator_host(E.bin_h(cid), c.J, c.L, c.Z), 300)


@pytest.mark.parametrize("cid", E.NB_IDS)
def test_nb_generator_stand_alone(nb, gen_exe, cid):
    mpath, gpath = E.nb_files(cid)
    mul, _, _ = nb.GFInitial(E.nb_code(cid).q, gpath)
    _run(gen_exe, ["nb", mpath, gpath], nb.generator_host(nb.NBMatrix(mpath), mul), 300)


def test_threaded_passes_on_the_large_shipped_matrices(C, nb, gen_exe):
    """J15_L30_Z1280 (parallel_for's clearing pass) and Tanner_74_9_Z128_GF16 (the elimination's SpinBarrier with its double-buffered
    sel / sel_hi slot) are the two codes on which the generators spawn threads."""
    path = os.path.join(DATA, "bldpc", "J15_L30_Z1280_BlockH.txt")
    H, _, _ = C.Get_H(path, 15, 30)
    threads = _run(gen_exe, ["b", path, 15, 30, 1280], C.generator_host(H, 15, 30, 1280), 900)
    mpath = os.path.join(DATA, "nb", "Tanner_74_9_Z128_GF16.txt")
    gpath = os.path.join(DATA, "nb", "GF", "Arith.Table.GF.16.txt")
    mul, _, _ = nb.GFInitial(16, gpath)
    Hn = nb.NBMatrix(mpath)
    assert 19200 * 300 >= 1 << 20 and Hn.M * Hn.N >= 1 << 20, "the sizes from which both generators go parallel"
    assert _run(gen_exe, ["nb", mpath, gpath], nb.generator_host(Hn, mul), 900) == threads
    if len(os.sched_getaffinity(0)) > 1:
        assert threads > 1, "the threaded passes ran on one thread: nothing for the race detector to see"
