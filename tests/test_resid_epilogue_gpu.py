"""The batched residual epilogue (SHOWO_EPI_RESID_F32: the residual loads of a group of fragments issued back to back, gemm_common.h
resid_tile_batched) against the per-fragment form it replaces and against the two roundings it stands for.

Every case runs one launch three ways in one process and compares bit for bit (torch.equal, no tolerance):
  new  = showo_gemm_set_resid_batch(1), old = showo_gemm_set_resid_batch(0): the WHOLE output allocations, pre-filled with a sentinel
         (the pad columns between rows of a strided output must survive);
  ref  = the same launch with SHOWO_EPI_F32 followed by an fp32 torch.add of the residual: fl(fl(acc + bias) + resid), the same two
         roundings in the same order.
Shapes: M = 549 (every tile height from 96 to 256 rows has full m-tiles and one ragged m-tile), K = 128, N = 512 (full n-tiles only),
320 (a ragged n-tile) and 322 (N % 4 != 0: with rows of 322 floats no 16-byte access at all, with padded rows the full n-tile takes the
batched form and the ragged one does not).  In place (out == resid, the engine's use) and out of place with ldr != ldo."""
import ctypes as C
import functools

import pytest
import torch

import util
from util import dev, to_bf16_bits

pytestmark = pytest.mark.gpu

F16 = 1  # SHOWO_OP_F16
EPI_F32, EPI_RESID = 2, 3
M = 549
ALL_VARIANTS = [256, 240, 224, 208, 176, 160, 144, 1192, 1176, 1160, 1144, 1128, 2256, 2240, 2224, 2208, 3192, 3176, 3160, 3144,
                4192, 4176, 4160, 4144]
# (N, ldo, ldr) of the out-of-place runs; the in-place runs use ldo for both
LAYOUTS = [(512, 520, 516), (320, 328, 324), (322, 322, 322), (322, 328, 324)]


def L():
    return util.lib()


def S():
    return util.lib().stream()


@functools.lru_cache(maxsize=None)
def _ops(N, K, half):
    """operands of one (N, K, type), made once: A [M, K], a second A of K columns in rows of K + 8, W [N, K], bias, residual [M, N]"""
    g = torch.Generator().manual_seed(N * 7 + K + (1 if half else 0))
    conv = (lambda t: t.to(torch.float16).view(torch.int16)) if half else to_bf16_bits
    A = torch.randn(M, K, generator=g)
    A1 = torch.zeros(M, K + 8)
    A1[:, :K] = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) * 0.05
    return {"A": dev(conv(A)), "A1": dev(conv(A1)), "W": dev(conv(W)), "bias": dev(torch.randn(N, generator=g)),
            "resid": torch.randn(M, N, generator=g).cuda()}


def _sentinel(rows, ld):
    return torch.full((rows, ld), -12345.678, dtype=torch.float32, device="cuda")


def _launch(o, N, K, epi, out, ldo, resid, ldr, half=False, kcat=0):
    """kcat = K0 > 0: the K-concatenated entry, columns [0, K0) from A (rows of K), the other K - K0 from A1 (rows of K + 8)"""
    p = L().ptr
    rp = p(resid) if resid is not None else None
    if kcat:
        L().call("showo_gemm_kcat_op16", p(o["A"]), K, kcat, p(o["A1"]), K + 8, K - kcat, p(o["W"]), K, p(o["bias"]), p(out), ldo, rp, ldr,
                 M, N, epi, 0, F16 if half else 0, S())
    else:
        L().call("showo_gemm_op16", p(o["A"]), K, p(o["W"]), K, p(o["bias"]), 0, p(out), ldo, rp, ldr, M, N, K, epi, F16 if half else 0, S())


def _resid_run(batch, o, N, K, ldo, ldr, inplace, **kw):
    """one residual launch with the switch at `batch`; returns the whole output allocation"""
    out = _sentinel(M, ldo)
    if inplace:
        out[:, :N] = o["resid"]
        resid, ldr = out, ldo
    else:
        resid = _sentinel(M, ldr)
        resid[:, :N] = o["resid"]
    L().call("showo_gemm_set_resid_batch", batch)
    try:
        _launch(o, N, K, EPI_RESID, out, ldo, resid, ldr, **kw)
        torch.cuda.synchronize()
    finally:
        L().call("showo_gemm_set_resid_batch", -1)
    if not inplace:
        assert torch.equal(resid[:, N:], _sentinel(M, ldr)[:, N:]) and torch.equal(resid[:, :N], o["resid"]), "the residual was written"
    return out


def _reference(o, N, K, half=False, kcat=0):
    """fl(fl(acc + bias) + resid): the plain fp32 epilogue of the same launch, then torch's fp32 add.  The K-concatenated entry has the
    residual epilogue only; its product is that of one A with the same K columns (the same k order per output element)."""
    if kcat:
        A = torch.cat([o["A"][:, :kcat], o["A1"][:, :K - kcat]], 1).contiguous()
        o = dict(o, A=A)
    plain = torch.empty(M, N, dtype=torch.float32, device="cuda")
    _launch(o, N, K, EPI_F32, plain, N, None, 0, half=half)
    torch.cuda.synchronize()
    return plain + o["resid"]


def _check(o, N, K, ldo, ldr, ref, **kw):
    for inplace in (True, False):
        old = _resid_run(0, o, N, K, ldo, ldr, inplace, **kw)
        new = _resid_run(1, o, N, K, ldo, ldr, inplace, **kw)
        assert torch.equal(old, new), f"N {N} ldo {ldo} inplace {inplace}: batched form differs from the per-fragment form"
        assert torch.equal(new[:, N:], _sentinel(M, ldo)[:, N:]), "the pad between rows was written"
        assert torch.equal(new[:, :N], ref), f"N {N} ldo {ldo} inplace {inplace}: not fl(fl(acc + bias) + resid)"


@pytest.fixture
def variant(request):
    L().call("showo_gemm_tune", 8, request.param << 8, None)
    yield request.param
    L().call("showo_gemm_tune", 8, 0, None)


@pytest.mark.parametrize("variant", ALL_VARIANTS, indirect=True)
def test_resid_batched_equals_per_fragment_and_two_roundings(variant):
    K = 128
    for N, ldo, ldr in LAYOUTS:
        o = _ops(N, K, False)
        _check(o, N, K, ldo, ldr, _reference(o, N, K))


@pytest.mark.parametrize("variant", [4160, 3192, 2208, 1160, 256], indirect=True)
def test_resid_batched_kcat_entry(variant):
    """showo_gemm_kcat_op16 with Ksplit 64 + 128 and a second A with its own leading dimension"""
    K = 192
    for N, ldo, ldr in LAYOUTS:
        o = _ops(N, K, False)
        _check(o, N, K, ldo, ldr, _reference(o, N, K, kcat=64), kcat=64)


@pytest.mark.parametrize("variant", [4160, 3192, 2208, 1160, 256], indirect=True)
def test_resid_batched_fp16_operands(variant):
    K = 128
    for N, ldo, ldr in LAYOUTS:
        o = _ops(N, K, True)
        _check(o, N, K, ldo, ldr, _reference(o, N, K, half=True), half=True)
    o = _ops(512, 192, True)
    _check(o, 512, 192, 520, 516, _reference(o, 512, 192, half=True, kcat=64), half=True, kcat=64)


def _splits():
    out = (C.c_int64 * 3)()
    L().call("showo_gemm_counters", C.cast(out, C.c_void_p), 1)
    return int(out[2])


@pytest.mark.parametrize("variant", [0, 256, 176, 1160], indirect=True)
def test_resid_batched_split_k_shape(variant):
    """K = 2048 at 6 tiles: the launch splits K in two (the policy is a function of the problem); both finish paths keep their bits"""
    K, N = 2048, 512
    o = _ops(N, K, False)
    _splits()
    ref = _reference(o, N, K)
    assert _splits() == 1, "the shape did not take split-K"
    _check(o, N, K, 520, 516, ref)
    assert _splits() == 4

