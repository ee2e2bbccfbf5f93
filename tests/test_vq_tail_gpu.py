"""The low-power tail of the VQ decode / encode: the attention block as one strided batch over the images, the strided-batch split
GEMM entry on its own, the GroupNorm apply pass with a grid sized to the tensor, and the finalize pass folded into the apply kernel.
Every one of these promises the BITS of the form it replaces, so the checks are torch.equal against that form (selected through the
library's switches in the same process); the GroupNorm output is also held to test_groupnorm_and_conv's bound against an fp64
reference.  The thin-Cout conv of decoder.conv_out and split-K on the 3-tap conv kernel change the summation order: they are held to
the split kernels' bound, 3e-5 of the output scale against an fp64 convolution of the unrounded operands."""
import ctypes as C

import pytest
import torch

import util
from util import O, Wt, dev, from_bf16_bits

pytestmark = pytest.mark.gpu


def L():
    return util.lib()


def S():
    return util.lib().stream()


def _split(t):
    """(hi, lo) bf16 bit tensors on the device with t ~= hi + lo"""
    hi = torch.empty(t.shape, dtype=torch.int16, device="cuda")
    lo = torch.empty_like(hi)
    src = dev(t)
    L().call("showo_split_f32_bf16", L().ptr(src), L().ptr(hi), L().ptr(lo), t.numel(), S())
    torch.cuda.synchronize()
    return hi, lo


# ------------------------------------------------------------------------------------ attention block
@pytest.fixture(scope="module")
def magvit():
    v = util.pkg().MAGVITv2(max_batch=3, max_res=192, precision=1)
    v.load_state_dict(O.to_torch(Wt.make_magvit_state(seed=5)), strict=True)
    return v.cuda().eval()


@pytest.mark.parametrize("lat", [4, 8, 12])  # hw = 16 (hwp = 64: padded key columns), 64 (no padding), 144 (hwp = 192)
def test_batched_attention_block_equals_the_loop_through_decode_code(magvit, lat):
    g = torch.Generator().manual_seed(lat)
    ids = torch.randint(0, 2 ** 13, (3, lat * lat), generator=g).cuda()
    for B in (1, 3):
        magvit.set_tail(attn_batched=True)
        img = magvit.decode_code(ids[:B])
        magvit.set_tail(attn_batched=False)
        loop = magvit.decode_code(ids[:B])
        magvit.set_tail(attn_batched=True)
        assert torch.isfinite(img).all()
        assert torch.equal(img, loop), (lat, B)


@pytest.mark.parametrize("lat", [4, 8, 12])
def test_batched_attention_block_equals_the_loop_and_single_image_calls(magvit, lat):
    """The block on its own (showo_vq_attn_block, in place on a [B, hw, 512] activation): batched == loop == B single-image calls,
    bitwise.  (Through decode_code the single-image comparison is not available: the split-K count of the convolutions around the block
    follows the launch's tile count, so a batch of 3 and three batches of 1 differ in the convs' low bits, with the loop form as well.)"""
    vq = magvit.engine()
    hw, Cc = lat * lat, 512
    x = (torch.randn(3, hw, Cc, generator=torch.Generator().manual_seed(lat)) * 1.5 + 0.1).cuda()

    def run(xin, batched):
        y = xin.clone()
        magvit.set_tail(attn_batched=batched)
        try:
            L().call("showo_vq_attn_block", vq, b"decoder.mid.attn_1", L().ptr(y), y.shape[0], lat, lat, S())
            torch.cuda.synchronize()
        finally:
            magvit.set_tail(attn_batched=True)
        return y

    for B in (1, 3):
        got = run(x[:B], True)
        assert torch.isfinite(got).all() and not torch.equal(got, x[:B])
        assert torch.equal(got, run(x[:B], False)), (lat, B)
        assert torch.equal(got, torch.cat([run(x[b:b + 1], True) for b in range(B)])), (lat, B)


def test_batched_attention_block_in_the_encoder(magvit):
    """get_code runs the same block: ids and latents of the batched form equal the loop form's"""
    g = torch.Generator().manual_seed(9)
    px = (torch.rand(3, 3, 64, 64, generator=g) * 2 - 1).cuda()
    magvit.set_tail(attn_batched=True)
    ids, z = magvit.get_code_and_latents(px)
    magvit.set_tail(attn_batched=False)
    ids2, z2 = magvit.get_code_and_latents(px)
    magvit.set_tail(attn_batched=True)
    assert torch.equal(ids, ids2) and torch.equal(z, z2)


# ------------------------------------------------------------------------------------ strided-batch GEMM
@pytest.mark.parametrize("M,N,K,ldo,per_row,resid", [(64, 64, 128, 64, False, False), (144, 144, 512, 160, False, False),
                                                      (144, 144, 512, 144, True, False), (64, 64, 128, 72, False, True)])
def test_strided_batch_split_gemm_equals_single_launches_and_stays_inside_its_outputs(M, N, K, ldo, per_row, resid):
    torch.manual_seed(M + K + ldo)
    nb, guard = 3, 256
    A, W = torch.randn(nb, M, K), torch.randn(nb, N, K) * 0.05
    bias = torch.randn(nb, M if per_row else N)
    Ah, Al = _split(A)
    Wh, Wl = _split(W)
    bd = dev(bias)
    sO = M * ldo + 8  # a gap between the images' outputs as well
    res = torch.randn(nb * sO + 2 * guard, device="cuda") if resid else None
    out = torch.full((nb * sO + 2 * guard,), float("nan"), device="cuda")
    o0 = out[guard:]
    r0 = None if res is None else res[guard:]
    L().call("showo_gemm_bf16x3_batched", L().ptr(Ah), L().ptr(Al), K, M * K, L().ptr(Wh), L().ptr(Wl), K, N * K, L().ptr(bd),
             int(per_row), bias.shape[1], L().ptr(o0), ldo, sO, None if r0 is None else L().ptr(r0), ldo, sO, M, N, K, nb, S())
    torch.cuda.synchronize()
    written = torch.zeros_like(out, dtype=torch.bool)
    for z in range(nb):
        one = torch.full((M, ldo), float("nan"), device="cuda")
        rz = None if r0 is None else r0[z * sO:z * sO + M * ldo]
        L().call("showo_gemm_bf16x3", L().ptr(Ah[z]), L().ptr(Al[z]), K, L().ptr(Wh[z]), L().ptr(Wl[z]), K, L().ptr(bd[z]), int(per_row),
                 L().ptr(one), ldo, None if rz is None else L().ptr(rz), ldo, M, N, K, S())
        torch.cuda.synchronize()
        got = o0[z * sO:z * sO + M * ldo].reshape(M, ldo)
        assert torch.isfinite(got[:, :N]).all()
        assert torch.equal(got[:, :N], one[:, :N]), z
        written[guard + z * sO:guard + z * sO + M * ldo].reshape(M, ldo)[:, :N] = True
    assert torch.isnan(out[~written]).all()  # guard bands, row padding (ldo > N) and the gaps between images are untouched
    # the shared-operand form (stride 0), as the attention block's V^T product uses it: every image sees image 0's A
    out2 = torch.full((nb, M, ldo), float("nan"), device="cuda")
    L().call("showo_gemm_bf16x3_batched", L().ptr(Ah), L().ptr(Al), K, 0, L().ptr(Wh), L().ptr(Wl), K, N * K, L().ptr(bd), int(per_row), 0,
             L().ptr(out2), ldo, M * ldo, None, ldo, 0, M, N, K, nb, S())
    one = torch.full((M, ldo), float("nan"), device="cuda")
    L().call("showo_gemm_bf16x3", L().ptr(Ah[0]), L().ptr(Al[0]), K, L().ptr(Wh[2]), L().ptr(Wl[2]), K, L().ptr(bd[0]), int(per_row),
             L().ptr(one), ldo, None, ldo, M, N, K, S())
    torch.cuda.synchronize()
    assert torch.equal(out2[2, :, :N], one[:, :N])
    assert L().load().showo_gemm_bf16x3_batched(L().ptr(Ah), L().ptr(Al), K, 4, L().ptr(Wh), L().ptr(Wl), K, N * K, None, 0, 0, L().ptr(out2),
                                                ldo, M * ldo, None, ldo, 0, M, N, K, nb, S()) != 0  # operand stride not a multiple of 8


# ------------------------------------------------------------------------------------ GroupNorm apply
def _gn_apply(x, stats, gam, bet, B, HW, Cc, swish, split):
    y = torch.full((B, HW, Cc), 0x7fc0, dtype=torch.int16, device="cuda")
    ylo = torch.full_like(y, 0x7fc0) if split else None
    L().call("showo_gn_apply", L().ptr(x), L().ptr(stats), L().ptr(gam), L().ptr(bet), L().ptr(y), None if ylo is None else L().ptr(ylo),
             B, HW, Cc, 1e-6, int(swish), S())
    torch.cuda.synchronize()
    return y, ylo


@pytest.mark.parametrize("Cc", [128, 512])
@pytest.mark.parametrize("HW", [256, 520, 1024, 4096])
def test_gn_apply_grid_sized_to_the_tensor_keeps_the_bits_of_the_fixed_grid(HW, Cc):
    import torch.nn.functional as F
    torch.manual_seed(HW + Cc)
    Bmax = 3
    x = torch.randn(Bmax, HW, Cc) * 2 + 0.3
    gam, bet = torch.randn(Cc) * .1 + 1, torch.randn(Cc) * .05
    xd, gd, bd = dev(x), dev(gam), dev(bet)
    gn64 = F.group_norm(x.double().permute(0, 2, 1), 32, gam.double(), bet.double(), eps=1e-6).permute(0, 2, 1)  # CPU, fp64, once
    want = {0: gn64, 1: gn64 * torch.sigmoid(gn64)}
    for B in (1, 3):
        stats = torch.zeros((L().load().showo_gn_stats_doubles(B, HW),), dtype=torch.float64, device="cuda")
        L().call("showo_gn_stats", L().ptr(xd), L().ptr(stats), B, HW, Cc, S())
        for swish in (0, 1):
            for split in (False, True):
                try:
                    L().call("showo_gn_set_fixed_grid", 1)
                    y0, l0 = _gn_apply(xd, stats, gd, bd, B, HW, Cc, swish, split)
                finally:
                    L().call("showo_gn_set_fixed_grid", 0)
                y1, l1 = _gn_apply(xd, stats, gd, bd, B, HW, Cc, swish, split)
                assert torch.equal(y0, y1), (B, swish, split)
                w = want[swish][:B]
                got = from_bf16_bits(y1).cpu().double()
                assert (got - w).abs().max() < 2 ** -8 * float(w.abs().max()) + 1e-5  # test_groupnorm_and_conv's bounds
                if split:
                    assert torch.equal(l0, l1), (B, swish)
                    got2 = got + from_bf16_bits(l1).cpu().double()
                    assert (got2 - w).abs().max() < 3e-5 * float(w.abs().max())


# ------------------------------------------------------------------------------------ folded finalize
def _apply_pair_and_folded(x, stats, nblk, gam, bet, B, HW, Cc):
    """(y, ylo) of showo_gn_finalize + showo_gn_apply and of showo_gn_apply_part on the same partials"""
    part = stats[B * 64:]
    L().call("showo_gn_finalize", L().ptr(part), L().ptr(stats), B, nblk, S())
    ref = _gn_apply(x, stats, gam, bet, B, HW, Cc, 1, True)
    stats[:B * 64] = float("nan")  # the folded form must not read the summed statistics
    y = torch.full((B, HW, Cc), 0x7fc0, dtype=torch.int16, device="cuda")
    ylo = torch.full_like(y, 0x7fc0)
    L().call("showo_gn_apply_part", L().ptr(x), L().ptr(part), nblk, L().ptr(gam), L().ptr(bet), L().ptr(y), L().ptr(ylo), B, HW, Cc, 1e-6, 1, S())
    torch.cuda.synchronize()
    return ref, (y, ylo)


@pytest.mark.parametrize("nblk", [1, 4, 16])
def test_gn_apply_from_partials_equals_finalize_then_apply(nblk):
    torch.manual_seed(nblk)
    lib = L().load()
    B, Cc = 3, 128
    gam, bet = dev(torch.randn(Cc) * .1 + 1), dev(torch.randn(Cc) * .05)
    # (a) partials of showo_gn_stats: one per 512 pixels (a ragged last block when nblk > 1)
    HW = 512 * nblk - (40 if nblk > 1 else 0)
    x = dev(torch.randn(B, HW, Cc) * 2 + 0.3)
    stats = torch.full((lib.showo_gn_stats_doubles(B, HW) + 64 * B * nblk,), float("nan"), dtype=torch.float64, device="cuda")
    pend = C.c_int(-1)
    L().call("showo_gn_stats_lazy", L().ptr(x), L().ptr(stats), B, HW, Cc, C.byref(pend), S())
    assert pend.value == nblk
    ref, got = _apply_pair_and_folded(x, stats, nblk, gam, bet, B, HW, Cc)
    assert torch.equal(ref[0], got[0]) and torch.equal(ref[1], got[1])
    full = torch.zeros_like(stats)
    L().call("showo_gn_stats", L().ptr(x), L().ptr(full), B, HW, Cc, S())
    y2, l2 = _gn_apply(x, full, gam, bet, B, HW, Cc, 1, True)
    assert torch.equal(y2, got[0]) and torch.equal(l2, got[1])  # and the bits of the two-launch statistics path
    # (b) partials of the conv epilogue: one per 256-pixel tile, Hout * Wout = 256 * nblk
    H, W = {1: (16, 16), 4: (32, 32), 16: (64, 64)}[nblk]
    Cin = 64
    xh, xl = _split(torch.randn(B, H, W, Cin) + 0.2)
    wh, wl = _split(torch.randn(Cc, 3, 3, Cin) * 0.03)
    bias = dev(torch.randn(Cc))
    out = torch.full((B, H * W, Cc), float("nan"), device="cuda")
    stats = torch.full((lib.showo_gn_stats_doubles(B, H * W),), float("nan"), dtype=torch.float64, device="cuda")
    pend = C.c_int(-1)
    L().call("showo_conv3x3_bf16x3_gn_lazy", L().ptr(xh), L().ptr(xl), L().ptr(wh), L().ptr(wl), L().ptr(bias), None, L().ptr(out),
             L().ptr(stats), B, H, W, Cin, Cc, 0, C.byref(pend), S())
    assert pend.value == nblk, "the conv epilogue must have produced the partials"
    ref, got = _apply_pair_and_folded(out, stats, nblk, gam, bet, B, H * W, Cc)
    assert torch.equal(ref[0], got[0]) and torch.equal(ref[1], got[1])
    assert lib.showo_gn_apply_part(L().ptr(out), L().ptr(stats), 17, L().ptr(gam), L().ptr(bet), L().ptr(got[0]), None, B, H * W, Cc,
                                   C.c_float(1e-6), 1, S()) != 0  # more partials than the kernel folds


def test_decode_with_folded_finalize_equals_the_separate_launch(magvit):
    ids = torch.randint(0, 2 ** 13, (2, 16), generator=torch.Generator().manual_seed(3)).cuda()
    magvit.set_tail(gn_fold=True)
    img = magvit.decode_code(ids)
    magvit.set_tail(gn_fold=False)
    ref = magvit.decode_code(ids)
    magvit.set_tail(gn_fold=True)
    assert torch.isfinite(img).all() and torch.equal(img, ref)


# ------------------------------------------------------------------------------------ thin-Cout conv
@pytest.mark.parametrize("B,H,W", [(1, 16, 16), (2, 32, 16), (1, 8, 40), (1, 5, 150)])  # (the last: three segments, a ragged one)
def test_thin_cout_conv_tracks_fp64_and_stays_inside_its_output(B, H, W):
    """showo_conv3x3_thin_bf16x3 (decoder.conv_out's kernel) against an fp64 convolution of the original fp32 operands: 3e-5 of the
    output scale, the split kernels' bound (test_split_conv_three_tap_reuse_kernel_tracks_fp64_and_gn_statistics)."""
    import torch.nn.functional as F
    torch.manual_seed(B * 1000 + H * 10 + W)
    Cin, Cout, guard = 128, 3, 512
    x = torch.randn(B, H, W, Cin) + 0.2
    wgt = torch.randn(Cout, 3, 3, Cin) * 0.03
    bias = torch.randn(Cout)
    xh, xl = _split(x)
    wh, wl = _split(wgt)
    n = B * H * W * Cout
    buf = torch.full((n + 2 * guard,), float("nan"), device="cuda")
    L().call("showo_conv3x3_thin_bf16x3", L().ptr(xh), L().ptr(xl), L().ptr(wh), L().ptr(wl), L().ptr(dev(bias)), L().ptr(buf[guard:]),
             B, H, W, Cin, Cout, S())
    torch.cuda.synchronize()
    assert torch.isnan(buf[:guard]).all() and torch.isnan(buf[guard + n:]).all()  # the guard bands keep their sentinel
    out = buf[guard:guard + n].reshape(B, H, W, Cout).cpu()
    assert torch.isfinite(out).all()  # every output element was written
    ref = F.conv2d(x.permute(0, 3, 1, 2).double(), wgt.permute(0, 3, 1, 2).double(), bias.double(), padding=1).permute(0, 2, 3, 1)
    err = float((out.double() - ref).abs().max() / ref.abs().max())
    print(f"[thin conv] B={B} H={H} W={W}: err={err:.3e}")
    assert err < 3e-5, err
    buf2 = torch.full_like(buf, float("nan"))
    L().call("showo_conv3x3_thin_bf16x3", L().ptr(xh), L().ptr(xl), L().ptr(wh), L().ptr(wl), L().ptr(dev(bias)), L().ptr(buf2[guard:]),
             B, H, W, Cin, Cout, S())
    assert torch.equal(buf[guard:guard + n], buf2[guard:guard + n])  # same bits on every run


def test_thin_cout_conv_other_widths_and_channel_count_errors():
    import torch.nn.functional as F
    torch.manual_seed(4)
    lib = L().load()
    for Cin, Cout in ((32, 1), (96, 4), (256, 2)):
        B, H, W = 1, 6, 9
        x = torch.randn(B, H, W, Cin) + 0.2
        wgt = torch.randn(Cout, 3, 3, Cin) * 0.03
        xh, xl = _split(x)
        wh, wl = _split(wgt)
        out = torch.full((B, H, W, Cout), float("nan"), device="cuda")
        L().call("showo_conv3x3_thin_bf16x3", L().ptr(xh), L().ptr(xl), L().ptr(wh), L().ptr(wl), None, L().ptr(out), B, H, W, Cin, Cout, S())
        ref = F.conv2d(x.permute(0, 3, 1, 2).double(), wgt.permute(0, 3, 1, 2).double(), None, padding=1).permute(0, 2, 3, 1)
        err = float((out.cpu().double() - ref).abs().max() / ref.abs().max())
        assert err < 3e-5, (Cin, Cout, err)
    before = out.clone()
    for Cin, Cout in ((120, 3), (128, 5), (128, 0), (512, 3)):
        rc = lib.showo_conv3x3_thin_bf16x3(L().ptr(xh), L().ptr(xl), L().ptr(wh), L().ptr(wl), None, L().ptr(out), 1, 6, 9, Cin, Cout, S())
        assert rc == 1, (Cin, Cout, rc)  # the library's bad-argument code
        assert b"conv3x3 thin" in lib.showo_last_error()
    torch.cuda.synchronize()
    assert torch.equal(out, before)  # a refused call launches nothing


def test_decode_routes_conv_out_to_the_thin_kernel_within_the_split_bound(magvit):
    ids = torch.randint(0, 2 ** 13, (2, 16), generator=torch.Generator().manual_seed(8)).cuda()
    magvit.set_tail(thin_conv=True)
    img = magvit.decode_code(ids)
    magvit.set_tail(thin_conv=False)
    ref = magvit.decode_code(ids)
    magvit.set_tail(thin_conv=True)
    assert torch.isfinite(img).all()
    err = float((img - ref).abs().max() / ref.abs().max())
    print(f"[thin conv] decode 64x64: max|d| / max|ref| between the thin kernel and the MFMA conv = {err:.3e}")
    assert 0 < err < 6e-5  # each within 3e-5 of the exact convolution of the same operands; not the same bits (so the switch works)


# ------------------------------------------------------------------------------------ split-K on the 3-tap conv
SPLIT3_CASES = [(1, 16, 16, 128, 128, 0, True), (2, 16, 16, 512, 512, 0, False), (2, 32, 32, 256, 256, 0, True), (1, 16, 16, 128, 128, 1, False),
                (8, 16, 16, 512, 512, 0, True)]  # (B, H, W, Cin, Cout, mode, resid); the last is the production 16 x 16 shape


@pytest.mark.parametrize("B,H,Wd,Cin,Cout,mode,with_res", SPLIT3_CASES)
def test_split_k_three_tap_conv_tracks_fp64_with_statistics_and_clean_tickets(B, H, Wd, Cin, Cout, mode, with_res):
    """conv3t_split_kernel with splits > 1 (the 16 x 16 / 32 x 32 levels: few tiles, long K).  Against an fp64 convolution of the
    unrounded fp32 operands: 3e-5 of the output scale, the bound of test_split_conv_three_tap_reuse_kernel_tracks_fp64_and_gn_statistics;
    epilogue statistics against showo_gn_stats of the stored tensor; repeated launches on the stream's one split-K workspace give the
    same bits into NaN-filled buffers, which they can only do if every launch left the tiles' tickets at zero (a stale ticket makes a
    tile's last arriver miss: its outputs would keep the sentinel)."""
    import torch.nn.functional as F
    torch.manual_seed(B * 100 + Cin + mode)
    lib = L().load()
    Ho, Wo = (H, Wd) if mode == 0 else (2 * H, 2 * Wd)
    x = torch.randn(B, H, Wd, Cin) + 0.2
    wgt = torch.randn(Cout, 3, 3, Cin) * 0.03
    bias = torch.randn(Cout)
    res = torch.randn(B, Ho * Wo, Cout) if with_res else None
    xh, xl = _split(x)
    wh, wl = _split(wgt)
    bd = dev(bias)
    rd = None if res is None else dev(res)
    rp = None if rd is None else L().ptr(rd)
    nd = lib.showo_gn_stats_doubles(B, Ho * Wo)
    outs, sts = [], []
    n3, ns = lib.showo_conv3t_launches(), lib.showo_conv3t_split_launches()
    for rep in range(3):
        out = torch.full((B, Ho * Wo, Cout), float("nan"), dtype=torch.float32, device="cuda")
        st = torch.full((nd,), float("nan"), dtype=torch.float64, device="cuda")
        L().call("showo_conv3x3_bf16x3_gn", L().ptr(xh), L().ptr(xl), L().ptr(wh), L().ptr(wl), L().ptr(bd), rp, L().ptr(out),
                 L().ptr(st), B, H, Wd, Cin, Cout, mode, S())
        outs.append(out)
        sts.append(st)
    plain = torch.full((B, Ho * Wo, Cout), float("nan"), dtype=torch.float32, device="cuda")
    L().call("showo_conv3x3_bf16x3", L().ptr(xh), L().ptr(xl), L().ptr(wh), L().ptr(wl), L().ptr(bd), rp, L().ptr(plain), B, H, Wd, Cin, Cout,
             mode, S())
    torch.cuda.synchronize()
    assert lib.showo_conv3t_launches() == n3 + 4 and lib.showo_conv3t_split_launches() == ns + 4, "the case must split K on the 3-tap kernel"
    assert torch.isfinite(outs[0]).all()
    for o, s_ in zip(outs[1:], sts[1:]):
        assert torch.equal(outs[0], o) and torch.equal(sts[0][:B * 64], s_[:B * 64])
    assert torch.equal(outs[0], plain)
    xd = x.permute(0, 3, 1, 2).double()
    if mode == 1:
        xd = xd.repeat_interleave(2, 2).repeat_interleave(2, 3)
    ref = F.conv2d(xd, wgt.permute(0, 3, 1, 2).double(), bias.double(), padding=1).permute(0, 2, 3, 1).reshape(B, Ho * Wo, Cout)  # CPU, fp64
    if res is not None:
        ref = ref + res.double()
    err = float((outs[0].cpu().double() - ref).abs().max() / ref.abs().max())
    print(f"[split-K 3-tap] {(B, H, Wd, Cin, Cout, mode, with_res)}: err={err:.3e}")
    assert err < 3e-5, err
    st0 = torch.zeros((nd,), dtype=torch.float64, device="cuda")
    L().call("showo_gn_stats", L().ptr(outs[0]), L().ptr(st0), B, Ho * Wo, Cout, S())
    a, b = sts[0][:B * 64].cpu(), st0[:B * 64].cpu()
    assert torch.isfinite(a).all() and torch.allclose(a, b, rtol=1e-12, atol=1e-9), float((a - b).abs().max())
