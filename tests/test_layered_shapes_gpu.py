"""GPU tests of bldpc_decode_layered on random block matrices at the shapes the shipped matrices do not have (the table in
tests/test_layered_shapes_cpu.py): the partial last word and the ragged tiles of N % 64 != 0, k_lay_ws below and above its 256
threads, several frames in one wave that leave the iteration loop at different times, the LDS-state kernel with more than one
frame, 1024-thread workgroups, idle lanes in the last wave, block rows of weight 2, 3, 25 and 26, shifts 0 and Z - 1, every
`length` of the prefix rule.  The method is that of tests/test_layered_gpu.py: iters, flag row, hard bits and a-posteriori bit
patterns against bldpc_decode_layered_host, which test_layered_shapes_cpu.py holds against the numpy restatement on the same
matrices and the same input."""
import os

import numpy as np
import pytest
import torch

from conftest import DATA
from test_layered_cpu import special_inputs
from test_layered_shapes_cpu import SEVERAL_FRAMES_PER_WAVE, SHAPES, matrix_of, ramp_input, shape_id

pytestmark = pytest.mark.gpu

ACCEPTED = [s for s in SHAPES if s[5] is not None]
BY_DIMS = {s[:3]: s for s in SHAPES}
BATCHES = (1, 37)  # 37 leaves the last workgroup partly filled at 2, 4, 8 and 16 frames per workgroup


@pytest.fixture(scope="module")
def C():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_ldpc_amd
    return cuda_ldpc_amd


_codes, _inputs, _host = {}, {}, {}


def _code(C, s, fresh=False):
    J, L, Z = s[:3]
    if fresh:
        return C.BinaryCode.from_shifts(matrix_of(s), J, L, Z)
    if s[:3] not in _codes:
        _codes[s[:3]] = C.BinaryCode.from_shifts(matrix_of(s), J, L, Z)
    return _codes[s[:3]]


def _input(s, kind, F):
    """(host array, device tensor) of the shape's input: computed once, shared, never written to."""
    key = (s[:3], kind, F)
    if key not in _inputs:
        N = s[1] * s[2]
        y = ramp_input(N, F) if kind == "ramp" else special_inputs(N, F, np.random.default_rng(7))
        y.setflags(write=False)
        _inputs[key] = (y, torch.from_numpy(y.copy()).cuda())
    return _inputs[key]


def _want(C, s, kind, F, **kw):
    """The host decoder's result: computed once per case, shared among the tests."""
    key = (s[:3], kind, F, tuple(sorted(kw.items())))
    if key not in _host:
        J, L, Z = s[:3]
        _host[key] = C.layered_host(matrix_of(s), J, L, Z, _input(s, kind, F)[0], **kw)
    return _host[key]


def _same(code, r, want, what):
    assert np.array_equal(r["iters"].cpu().numpy(), want["iters"]), "iters: " + what
    D = r["D"].cpu().numpy()
    assert np.array_equal(D[code.N], want["D"][code.N]), "flag row: " + what
    assert np.array_equal(D[:code.N], want["D"][:code.N]), "hard bits: " + what
    assert np.array_equal(r["app"].cpu().numpy().view(np.uint32), want["app"].view(np.uint32)), "a-posteriori bits: " + what


def _both(C, s, kind, F, code=None, **kw):
    """The device and the host decoder on the same input: all outputs must carry the same bits."""
    code = code or _code(C, s)
    r = C.LDPC_Decoder_Layered_GPU(code, _input(s, kind, F)[1], want_app=True, **kw)
    torch.cuda.synchronize()
    want = _want(C, s, kind, F, **kw)
    _same(code, r, want, "%s %s F=%d %s" % (shape_id(s), kind, F, kw))
    return r, want


def _rules(C, s):
    N, K = s[1] * s[2], (s[1] - s[0]) * s[2]
    return [dict(stop_rule=C.STOP_SYNDROME)] + [dict(stop_rule=C.STOP_PREFIX, length=n) for n in (0, 1, K - 1, N)]


@pytest.mark.parametrize("s", ACCEPTED, ids=shape_id)
def test_random_shapes_match_host(C, s):
    code = _code(C, s)
    N = code.N
    for F in BATCHES:
        for alpha in (1.0, 0.75):
            for mode, max_iter in ((C.EXIT_FIXED, 5), (C.EXIT_PER_FRAME, 10)):
                for rule in _rules(C, s):
                    r, want = _both(C, s, "ramp", F, max_iter=max_iter, alpha=alpha, exit_mode=mode, **rule)
                    assert code.last_kernel == s[5], "%s ran %s" % (shape_id(s), code.last_kernel)
                    if mode != C.EXIT_PER_FRAME or F == 1 or rule.get("length", 0) not in (0, N):
                        continue
                    # conditions on the input, judged by the host statement: frames that stop and frames that never do; where
                    # several frames share a wave, at least three iteration counts, so that lanes of one wave really diverge
                    it = want["iters"]
                    assert (it == max_iter).any() and (it < max_iter).any(), "%s %s: iters %s" % (shape_id(s), rule, it)
                    if s[:3] in SEVERAL_FRAMES_PER_WAVE:
                        assert np.unique(it).size >= 3, "%s %s: iters %s" % (shape_id(s), rule, it)


@pytest.mark.parametrize("dims", [(3, 9, 50), (4, 24, 8), (5, 12, 32), (4, 27, 64)], ids=lambda d: "J%d_L%d_Z%d" % d)
def test_special_values_on_every_tier(C, dims):
    """Zeros of both signs, denormals, 2^100 and exact ties of two and of many minima (frame 0: every magnitude ties) on one shape
    of every tier; on (4, 27, 64) the ties meet the block rows of weight 2, 3 and 26."""
    s = BY_DIMS[dims]
    code = _code(C, s)
    if dims == (4, 27, 64):
        assert {2, 3, 26} <= set((matrix_of(s) != -1).sum(1).tolist())
    for alpha in (1.0, 0.75, 0.8):
        _both(C, s, "special", 8, max_iter=5, alpha=alpha)
    _both(C, s, "special", 8, max_iter=5, alpha=0.8, exit_mode=C.EXIT_PER_FRAME, stop_rule=C.STOP_SYNDROME)
    assert code.last_kernel == s[5]


def test_caller_provided_D_on_another_stream(C):
    s = BY_DIMS[(5, 12, 96)]
    code = _code(C, s)
    kw = dict(max_iter=10, alpha=0.75, exit_mode=C.EXIT_PER_FRAME, stop_rule=C.STOP_SYNDROME)
    r0, want = _both(C, s, "ramp", 37, **kw)
    yt = _input(s, "ramp", 37)[1]
    D = torch.full((code.N + 1, 37), -7, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())  # D is filled and yt uploaded on the current stream
    r = C.LDPC_Decoder_Layered_GPU(code, yt, D=D, want_app=True, stream=stream, **kw)
    stream.synchronize()
    assert r["D"] is D
    _same(code, r, want, "D= and stream=")
    assert torch.equal(r["D"], r0["D"]) and torch.equal(r["iters"], r0["iters"])
    assert torch.equal(r["app"].view(torch.int32), r0["app"].view(torch.int32))


@pytest.mark.parametrize("dims", [(3, 9, 96), (5, 12, 32)], ids=lambda d: "J%d_L%d_Z%d" % d)
def test_scratch_that_shrinks_and_grows(C, dims):
    """One code object of its own, whose scratch is sized by the largest call: 37 frames, then 1, then 37 again (the workspace
    kernel's row states move with F inside that scratch)."""
    s = BY_DIMS[dims]
    code = _code(C, s, fresh=True)
    kw = dict(max_iter=10, alpha=0.75, exit_mode=C.EXIT_PER_FRAME, stop_rule=C.STOP_SYNDROME)
    for F in (37, 1, 37):
        _both(C, s, "ramp", F, code=code, **kw)
        _both(C, s, "ramp", F, code=code, max_iter=5, alpha=1.0)
    assert code.last_kernel == s[5]
    code.close()


def test_refused_matrices(C):
    """Weight 27: the code object is not made (its limit of 26 blocks per block row is the layered decoder's own).  A refusal
    the layered decoder makes itself, a block row of weight 1: the same answer on the second call, and the flooding decoder of
    the same code object decodes as before."""
    from cuda_ldpc_amd._lib import LdpcError
    s = SHAPES[-1]
    assert s[5] is None and (matrix_of(s) != -1).sum(1).max() == 27
    for _ in range(2):
        with pytest.raises(LdpcError, match=r"\(-5\): .*\S"):
            _code(C, s, fresh=True)
    J, L, Z = 4, 24, 96
    H, _, _ = C.Get_H(os.path.join(DATA, "bldpc", "J4_L24_Z96_BlockH.txt"), J, L)
    H = H.copy().reshape(J, L)
    H[2, 1:] = -1
    H[2, 0] = 0
    thin = C.BinaryCode.from_shifts(H.reshape(-1), J, L, Z)
    y = torch.from_numpy(ramp_input(L * Z, 5)).cuda()

    def flood():
        r = C.LDPC_Decoder_GPU(thin, y, max_iter=8, exit_mode=C.EXIT_FIXED)
        torch.cuda.synchronize()
        return r["D"].clone()

    d0 = flood()
    said = []
    for _ in range(2):
        with pytest.raises(LdpcError, match=r"\(-5\): .*weight 1\b.*") as e:
            C.LDPC_Decoder_Layered_GPU(thin, y)
        said.append(str(e.value))
    assert said[0] == said[1]
    assert torch.equal(flood(), d0)
    thin = C.BinaryCode.from_shifts(H.reshape(-1), J, L, Z)  # and as a code object does that never saw a layered call
    assert torch.equal(flood(), d0)
