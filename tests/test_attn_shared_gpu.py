"""Shared-prefix decode attention (csrc/attn_shared.hip) through its test hooks: showo_attn_decode_shared runs one layer's prefix launch
and suffix + merge launch on caller buffers, showo_kv_copy_rows the row-range copy that fills a suffix cache.

Shapes: 2 heads of 64, rotary 32, prefixes P in {1, 63, 64, 65, 607} (one key, the edges of a 64-key split, the cfg4 prefix: ten splits),
nb in {1, 9, 16, 17, 32} slots, suffixes of 1 (only the new token) .. 70 rows so that P - base + suffix crosses a 64-row tile.  Everything
at or behind the live lengths holds NaN bits: prefix K rows and V^T columns >= P, the dead rows below P - base of every suffix cache, and
every row / column from a slot's position on (the launch itself writes the row at the position)."""
import ctypes as C

import pytest
import torch

import util

pytestmark = pytest.mark.gpu

NH, D, ROT, EPS = 2, 64, 32, 1e-5
PS = (1, 63, 64, 65, 607)
NBS = (1, 9, 16, 17, 32)
CAP_S = 192  # 63 dead rows + 70 suffix rows + room
NAN16 = 0x7FC0
SENT16, SENTF = 0x5A5A, -12345.0


def _L():
    return util.lib()


def _bits(t):
    """fp32 values that are exact in bf16 (or to be rounded) -> int16 bit patterns"""
    return util.to_bf16_bits(t.float())


def _vals(t):
    return util.from_bf16_bits(t.cpu()).double()


def _i16(v):
    return v - 65536 if v >= 32768 else v


class Case:
    """Buffers of one launch pair.  `suf_len[b]` counts the slot's suffix rows including the new token; K / V values are given as fp32
    tensors exact in bf16: kpre [NH, P, 64], vpre [NH, P, 64], ksuf / vsuf lists of [NH, suf_len[b] - 1, 64], xq / xk / xv [nb, NH, 64]
    (the new tokens' projection rows)."""

    def __init__(self, P, suf_len, kpre, vpre, ksuf, vsuf, xq, xk, xv, ln, iv):
        self.P, self.nb, self.base = P, len(suf_len), P & ~63
        self.suf_len = list(suf_len)
        self.pos = [P + s - 1 for s in suf_len]
        self.cap_p = (P + 63) // 64 * 64 + 64
        nb, cap_p = self.nb, self.cap_p
        kp = torch.full((NH, cap_p, D), _i16(NAN16), dtype=torch.int16)
        vp = torch.full((NH, D, cap_p), _i16(NAN16), dtype=torch.int16)
        kp[:, :P] = _bits(kpre)
        vp[:, :, :P] = _bits(vpre).transpose(1, 2)
        ks = torch.full((nb, NH, CAP_S, D), _i16(NAN16), dtype=torch.int16)
        vs = torch.full((nb, NH, D, CAP_S), _i16(NAN16), dtype=torch.int16)
        lo = P - self.base
        for b in range(nb):
            n = suf_len[b] - 1
            if n:
                ks[b, :, lo:lo + n] = _bits(ksuf[b])
                vs[b, :, :, lo:lo + n] = _bits(vsuf[b]).transpose(1, 2)
        qkv = torch.cat([_bits(x).reshape(nb, NH * D) for x in (xq, xk, xv)], dim=1)
        self.qw, self.qb, self.kw, self.kb = [t.float() for t in ln]
        maxpos = P + 80
        ang = torch.arange(maxpos, dtype=torch.float64)[:, None] * (1.0 / (10000.0 ** (torch.arange(ROT // 2, dtype=torch.float64) * 2 / ROT)))[None]
        ang = torch.cat([ang, ang], dim=1)
        self.cos, self.sin = ang.cos().float(), ang.sin().float()
        self.iv = [int(v) for v in iv]
        self.h = dict(kp=kp, vp=vp, ks=ks, vs=vs, qkv=qkv)
        self.kpre, self.vpre, self.ksuf, self.vsuf = kpre, vpre, ksuf, vsuf
        self.xv = util.bf16_round(xv.float())

    def upload(self):
        d = {k: v.cuda() for k, v in self.h.items()}
        d.update(qw=self.qw.cuda(), qb=self.qb.cuda(), kw=self.kw.cuda(), kb=self.kb.cuda(), cos=self.cos.cuda(), sin=self.sin.cuda(),
                 pos=torch.tensor(self.pos, dtype=torch.int32).cuda())
        return d

    def new_qk(self, d):
        """bf16 q (scaled) and k of every slot's new token as showo_qk_prep makes them: [nb, NH, 64] fp64 values, and the K bits"""
        L = _L()
        q = torch.empty((self.nb, NH, D), dtype=torch.float64)
        kbits = torch.empty((self.nb, NH, D), dtype=torch.int16)
        for b in range(self.nb):
            pos, lcap = self.pos[b], (self.pos[b] + 64) // 64 * 64
            Q = torch.zeros((NH, 1, D), dtype=torch.int16, device="cuda")
            K = torch.zeros((NH, lcap, D), dtype=torch.int16, device="cuda")
            Vt = torch.zeros((NH, D, lcap), dtype=torch.int16, device="cuda")
            row = d["qkv"][b:b + 1].contiguous()
            L.call("showo_qk_prep", L.ptr(row), L.ptr(d["qw"]), L.ptr(d["qb"]), L.ptr(d["kw"]), L.ptr(d["kb"]), L.ptr(d["cos"]),
                   L.ptr(d["sin"]), L.ptr(Q), L.ptr(K), L.ptr(Vt), 1, 1, NH, ROT, EPS, pos, lcap, lcap, L.stream())
            torch.cuda.synchronize()
            q[b] = _vals(Q[:, 0])
            kbits[b] = K[:, pos].cpu()
        return q, kbits

    def run(self, d=None, nb=None, O=None, ws=None):
        L = _L()
        d = d or self.upload()
        nb = nb or self.nb
        n_ws = L.load().showo_attn_shared_ws_elems(NH, self.P)
        assert n_ws == (self.P + 63) // 64 * NH * 32 * 68
        if O is None:
            O = torch.full((32, NH * D), _i16(SENT16), dtype=torch.int16, device="cuda")
        if ws is None:
            ws = torch.full((n_ws,), SENTF, dtype=torch.float32, device="cuda")
        iv = (C.c_int32 * 4)(*self.iv)
        L.call("showo_attn_decode_shared", L.ptr(d["qkv"]), L.ptr(d["qw"]), L.ptr(d["qb"]), L.ptr(d["kw"]), L.ptr(d["kb"]), L.ptr(d["cos"]),
               L.ptr(d["sin"]), L.ptr(d["kp"]), L.ptr(d["vp"]), self.cap_p, L.ptr(d["ks"]), L.ptr(d["vs"]), CAP_S,
               C.cast(iv, C.c_void_p), self.P, L.ptr(d["pos"]), max(self.pos) + 1, L.ptr(O), L.ptr(ws), nb, NH, ROT, EPS, L.stream())
        torch.cuda.synchronize()
        return O, ws, d

    def visible_prefix(self):
        a, b, c, e = self.iv
        k = torch.arange(self.P)
        return ((k >= a) & (k < min(b, self.P))) | ((k >= c) & (k < min(e, self.P)))

    def keys_values(self, b, knew):
        """(K [NH, n, 64], V [NH, n, 64]) fp64 of what slot b sees: visible prefix keys, its suffix rows, its new token"""
        vis = self.visible_prefix()
        ks = [self.kpre[:, vis].double()]
        vs = [self.vpre[:, vis].double()]
        if self.suf_len[b] > 1:
            ks.append(util.bf16_round(self.ksuf[b].float()).double())
            vs.append(util.bf16_round(self.vsuf[b].float()).double())
        ks.append(knew[b][:, None].double())
        vs.append(self.xv[b][:, None].double())
        return torch.cat(ks, dim=1), torch.cat(vs, dim=1)


def _ln(gen, zero_q=False, kscale=1.0, bias_hi=True):
    """random q / k LayerNorm weight and bias: weights of magnitude 1..2 with random signs, biases in +-0.5 (zero_q: the q pair is 0:
    every score is 0; kscale: the k pair is the q pair times it; bias_hi False: no bias on the dims 32..63, which the RoPE leaves alone)"""
    def w():
        return (1.0 + torch.rand(D, generator=gen)) * (torch.randint(0, 2, (D,), generator=gen) * 2 - 1)
    qw, qb, kw, kb = w(), torch.rand(D, generator=gen) - 0.5, w(), torch.rand(D, generator=gen) - 0.5
    if not bias_hi:
        qb[32:] = 0
        kb[32:] = 0
    if zero_q:
        qw, qb = torch.zeros(D), torch.zeros(D)
    if kscale != 1.0:
        kw, kb = qw * kscale, qb * kscale
    return qw, qb, kw, kb


def _suf_lens(nb, choices=None):
    if choices is not None:
        return [choices[b % len(choices)] for b in range(nb)]
    spread = [1, 70, 2, 64, 33, 65, 7, 50]  # 1 = only the new token; with P - base up to 63 the longer ones cross a 64-row tile
    return [spread[b % len(spread)] for b in range(nb)]


def _asym_v(nkeys, salt):
    """V [NH, nkeys, 64]: multiples of 0.5 below 128 (exact in bf16), distinct along keys and dims"""
    k = torch.arange(nkeys)[None, :, None]
    d = torch.arange(D)[None, None, :]
    h = torch.arange(NH)[:, None, None]
    return ((k * 7 + d * 13 + h * 3 + salt * 5) % 509 - 254).float() / 2


# ---- 1. index mapping ------------------------------------------------------------------------------------------------------------
def _candidates(P, s):
    """keys (absolute) a slot with s suffix rows can be pointed at: first prefix key, key P - 1, key P, the new token, one per split"""
    c = [0, P - 1]
    if s > 1:
        c.append(P)
    c.append(P + s - 1)
    c += [64 * i + min(17, P - 1 - 64 * i) for i in range((P + 63) // 64)]
    return c


@pytest.mark.parametrize("hide", [False, True])
@pytest.mark.parametrize("P", PS)
def test_a_dominating_key_returns_its_value_row_bit_for_bit(P, hide):
    """slot b's projection row is 8 at dim 32 + b, -0.25 on the dims 0..31 and 0 elsewhere: its mean is exactly 0, so without a bias
    there its query is exactly 0 on the other slots' dims 32 + b' and a key row may carry the one-hot of several slots.  The slot's
    primary key holds 300 / q at its dim, its secondary 150 / q, every other score is below ~1 (the new token: above 300 where it is
    the primary, below -250 elsewhere): every other p underflows to 0 (exp(-104) is below the smallest fp32 denormal) and the output
    is the primary's V row, or -- when the mask hides the primary -- the secondary's"""
    gen = torch.Generator().manual_seed(100 + P)
    for nb in NBS:
        suf = _suf_lens(nb)
        ln = _ln(gen, kscale=40.0, bias_hi=False)
        # hidden region [a, b) of the prefix: visible = [0, a) u [b, P)
        a, bnd = (P // 3, (2 * P + 2) // 3) if hide else (P, P)
        iv = (0, a, bnd, P)
        xq = torch.zeros((nb, NH, D))
        xq[:, :, :32] = -0.25
        xq[torch.arange(nb), :, 32 + torch.arange(nb)] = 8.0
        prim, sec = [], []
        for b in range(nb):
            cand = _candidates(P, suf[b])
            hidden = [k for k in cand if a <= k < bnd]
            seen = [k for k in cand if not (a <= k < bnd)]           # (the new token is always among them)
            seen_old = [k for k in seen if k != P + suf[b] - 1]
            if hidden and seen_old:                                   # a hidden primary, the secondary wins
                p, s2 = hidden[b % len(hidden)], seen_old[b % len(seen_old)]
            else:
                p = seen[b % len(seen)]
                rest = [k for k in seen_old if k != p]
                s2 = rest[b % len(rest)] if rest else None
            prim.append(p)
            sec.append(s2)
        # the new token dominates (x_k = x_q: k = 40 q / 0.125 up to rounding) where it is the primary, else it scores -300 or lower
        xk = torch.stack([xq[b] if prim[b] == P + suf[b] - 1 else -xq[b] for b in range(nb)])
        xv = _asym_v(nb, 3).permute(1, 0, 2).contiguous()
        kpre = (torch.rand((NH, P, D), generator=gen) - 0.5) * 0.25
        ksuf = [(torch.rand((NH, max(s - 1, 0), D), generator=gen) - 0.5) * 0.25 for s in suf]
        vpre = _asym_v(P, 0)
        vsuf = [_asym_v(max(s - 1, 0), 1 + b) for b, s in enumerate(suf)]
        c = Case(P, suf, kpre, vpre, ksuf, vsuf, xq, xk, xv, ln, iv)
        d = c.upload()
        q, _ = c.new_qk(d)
        for b in range(nb):  # the target rows: a one-hot at the slot's dim (rows shared by several slots hold all their dims)
            for key, score in ((prim[b], 300.0), (sec[b], 150.0)):
                if key is None or key == P + suf[b] - 1:
                    continue
                val = util.bf16_round((score / q[b, :, 32 + b]).float())
                if key < P:
                    kpre[:, key, 32 + b] = val
                else:
                    ksuf[b][:, key - P, 32 + b] = val
        c = Case(P, suf, kpre, vpre, ksuf, vsuf, xq, xk, xv, ln, iv)
        O, _, _ = c.run()
        got = O.cpu()[:nb].reshape(nb, NH, D)
        for b in range(nb):
            win = prim[b] if not (a <= prim[b] < bnd) else sec[b]
            assert win is not None
            if win < P:
                want = vpre[:, win]
            elif win == P + suf[b] - 1:
                want = c.xv[b]
            else:
                want = vsuf[b][:, win - P]
            assert torch.equal(got[b], _bits(want)), (P, nb, b, prim[b], sec[b], win)
        util.release()


# ---- 2. counting -----------------------------------------------------------------------------------------------------------------
def _count_cases(P):
    """(intervals, suffix lengths): visible prefix keys + suffix rows is a power of two <= 512 for every slot"""
    cases = [((0, 0, 0, 0), [1, 2, 4, 8, 16, 32, 64])]                       # empty prefix visibility: the suffix alone
    if P >= 64:
        cp = 60                                                               # two intervals; at P = 607 whole splits are hidden
        cases.append(((3, 33, P - 30, P), [4, 68]))
    else:
        cp = P
        cases.append(((0, P, 0, 0), [n - cp for n in (1, 2, 4, 8, 16, 32, 64, 128) if 1 <= n - cp <= 70]))
    if P == 607:
        cases.append(((0, 200, 359, 607), [64]))                              # 448 + 64 = 512 keys, every split visible or partly so
        cases.append(((130, 250, 0, 0), [8]))                                 # one interval inside: splits 0, 1 and 4..9 hidden whole
    return cases


@pytest.mark.parametrize("P", PS)
def test_counting_with_zero_scores_is_exact(P):
    """q LayerNorm weight and bias 0: every score is 0, every p is 1, V holds integers in [-8, 8] and the visible count is a power of
    two: the output is bf16(sum / count), bit for bit"""
    gen = torch.Generator().manual_seed(200 + P)
    for iv, choices in _count_cases(P):
        for nb in NBS:
            suf = _suf_lens(nb, choices)
            ri = lambda *shape: torch.randint(-8, 9, shape, generator=gen).float()
            kpre, vpre = torch.rand((NH, P, D), generator=gen) - 0.5, ri(NH, P, D)
            ksuf = [torch.rand((NH, s - 1, D), generator=gen) - 0.5 for s in suf]
            vsuf = [ri(NH, s - 1, D) for s in suf]
            xq, xk, xv = torch.randn((nb, NH, D), generator=gen), torch.randn((nb, NH, D), generator=gen), ri(nb, NH, D)
            c = Case(P, suf, kpre, vpre, ksuf, vsuf, xq, xk, xv, _ln(gen, zero_q=True), iv)
            O, _, _ = c.run()
            got = O.cpu()[:nb].reshape(nb, NH, D)
            nvis = int(c.visible_prefix().sum())
            for b in range(nb):
                count = nvis + suf[b]
                assert count & (count - 1) == 0 and 1 <= count <= 512, (P, iv, suf[b])
                _, V = c.keys_values(b, torch.zeros((nb, NH, D)))
                want = (V.sum(dim=1) / count).float()
                assert torch.equal(got[b], _bits(want)), (P, iv, nb, b, count)
            util.release()


# ---- 3. random operands against the fp64 soft-max ---------------------------------------------------------------------------------
def _softmax_ref(c, q, knew):
    out = torch.empty((c.nb, NH, D), dtype=torch.float64)
    for b in range(c.nb):
        K, V = c.keys_values(b, knew)
        s = torch.einsum("hd,hnd->hn", q[b], K)
        out[b] = torch.einsum("hn,hnd->hd", torch.softmax(s, dim=1), V)
    return out


@pytest.mark.parametrize("dominant", [False, True])
@pytest.mark.parametrize("P", PS)
def test_random_operands_against_the_fp64_softmax(P, dominant):
    """same bf16 q / K / V, two-interval visibility; gate 2.5 * 2^-8 * max|want| + 1e-3 (the gate of every attention kernel against this
    oracle, tests/test_kernels_gpu.py).  dominant: a key of the LAST prefix split scores 12 for slot 0 and a suffix key 12 for every odd
    slot (the others score ~ +-1.5), so the merge rescales by large factors in both directions"""
    gen = torch.Generator().manual_seed(300 + P)
    for nb in NBS:
        suf = _suf_lens(nb)
        kpre, vpre = torch.randn((NH, P, D), generator=gen), torch.randn((NH, P, D), generator=gen)
        ksuf = [torch.randn((NH, s - 1, D), generator=gen) for s in suf]
        vsuf = [torch.randn((NH, s - 1, D), generator=gen) for s in suf]
        xq, xk, xv = (torch.randn((nb, NH, D), generator=gen) for _ in range(3))
        iv = (0, max(P // 4, 1), P // 2, P)
        ln = _ln(gen)
        c = Case(P, suf, kpre, vpre, ksuf, vsuf, xq, xk, xv, ln, iv)
        d = c.upload()
        q, kb = c.new_qk(d)
        if dominant:
            late = P - 1 - (P - 1) % 64 + min(5, (P - 1) % 64)  # a key of the last split
            for b in range(nb):
                boost = util.bf16_round((12.0 * q[b] / (q[b] * q[b]).sum(dim=1, keepdim=True)).float())
                if b == 0:
                    kpre[:, late] = boost
                elif b % 2 == 1 and suf[b] > 1:
                    ksuf[b][:, (suf[b] - 2) // 2] = boost
            c = Case(P, suf, kpre, vpre, ksuf, vsuf, xq, xk, xv, ln, iv)
            d = c.upload()
        c.kpre, c.vpre = util.bf16_round(kpre), util.bf16_round(vpre)
        O, _, _ = c.run(d)
        got = _vals(O[:nb]).reshape(nb, NH, D)
        want = _softmax_ref(c, q, _vals(kb))
        err = float((got - want).abs().max())
        gate = 2.5 * 2.0 ** -8 * float(want.abs().max()) + 1e-3
        print(f"[attn_shared] P={P} nb={nb} dominant={dominant} err={err:.3e} gate={gate:.3e}")
        assert err <= gate, (P, nb, err, gate)
        util.release()


# ---- 4. independence ------------------------------------------------------------------------------------------------------------
def _random_case(P, nb, seed):
    gen = torch.Generator().manual_seed(seed)
    suf = _suf_lens(nb)
    r = lambda *s: torch.randn(s, generator=gen)
    return Case(P, suf, r(NH, P, D), r(NH, P, D), [r(NH, s - 1, D) for s in suf], [r(NH, s - 1, D) for s in suf], r(nb, NH, D),
                r(nb, NH, D), r(nb, NH, D), _ln(gen), (0, max(P // 4, 1), P // 2, P))


def _subset(c, slots):
    s = Case.__new__(Case)
    s.__dict__.update(c.__dict__)
    s.nb, s.suf_len, s.pos = len(slots), [c.suf_len[b] for b in slots], [c.pos[b] for b in slots]
    idx = torch.tensor(slots)
    s.h = dict(c.h, ks=c.h["ks"][idx].contiguous(), vs=c.h["vs"][idx].contiguous(), qkv=c.h["qkv"][idx].contiguous())
    return s


@pytest.mark.parametrize("P", PS)
def test_a_slot_does_not_depend_on_the_batch_and_rows_beyond_nb_are_untouched(P):
    full = _random_case(P, 32, 400 + P)
    O32, ws32, _ = full.run()
    rows = O32.cpu()
    assert not bool((rows[:32] == _i16(SENT16)).all(dim=1).any())
    for b in (0, 1, 8, 17, 31):  # alone: the nb = 1 launch
        O1, _, _ = _subset(full, [b]).run()
        assert torch.equal(O1.cpu()[0], rows[b]), (P, b)
    perm = torch.randperm(32, generator=torch.Generator().manual_seed(P)).tolist()
    Op, _, _ = _subset(full, perm).run()
    assert torch.equal(Op.cpu(), rows[perm]), P
    nsplit = (P + 63) // 64
    for nb in NBS[:-1]:  # the first nb slots: equal rows, sentinel behind them, in O and in the workspace
        On, wsn, _ = _subset(full, list(range(nb))).run()
        on = On.cpu()
        assert torch.equal(on[:nb], rows[:nb]), (P, nb)
        assert bool((on[nb:] == _i16(SENT16)).all()), (P, nb)
        w = wsn.cpu().reshape(nsplit, NH, 32, 68)
        assert bool((w[:, :, nb:] == SENTF).all()), (P, nb)
        assert torch.equal(w[:, :, :nb, :2], ws32.cpu().reshape(nsplit, NH, 32, 68)[:, :, :nb, :2]), (P, nb)
    util.release()


# ---- 5. the append -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", PS)
def test_the_launch_appends_what_qk_prep_writes_and_leaves_the_prefix_alone(P):
    c = _random_case(P, 17, 500 + P)
    d = c.upload()
    kp0, vp0, ks0, vs0 = (d[k].clone() for k in ("kp", "vp", "ks", "vs"))
    _, kbits = c.new_qk(d)
    c.run(d)
    assert torch.equal(d["kp"], kp0) and torch.equal(d["vp"], vp0)
    ks, vs = d["ks"].cpu(), d["vs"].cpu()
    want_k, want_v = ks0.cpu(), vs0.cpu()
    for b in range(c.nb):
        r = c.pos[b] - c.base
        want_k[b, :, r] = kbits[b]
        want_v[b, :, :, r] = _bits(c.xv[b])
    assert torch.equal(ks, want_k) and torch.equal(vs, want_v)  # the new row / column, nothing else
    util.release()


# ---- 6. the row copy -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 64])
@pytest.mark.parametrize("r0", [63, 64, 65])
def test_kv_copy_rows_is_a_bit_copy_of_the_range_that_writes_nothing_else(r0, n):
    """random 16-bit patterns (NaN / inf among them) in a source of capacity 256 with padded layer strides, a sentinel in the
    destination: rows [r0, r1) arrive at [r0 - base, r1 - base) bit for bit, V^T up to the end of the last tile is zero, everything
    else keeps the sentinel, the source is unchanged"""
    L = _L()
    nL, nH, cap_src, cap_dst = 2, 3, 256, 192
    base, r1 = r0 & ~63, r0 + n
    gen = torch.Generator().manual_seed(r0 * 100 + n)
    ks, vs = nH * cap_src * 64 + 64, nH * 64 * cap_src + 8
    kd, vd = nH * cap_dst * 64 + 8, nH * 64 * cap_dst + 64
    src_k = torch.randint(-32768, 32768, (nL * ks,), generator=gen, dtype=torch.int32).to(torch.int16)
    src_v = torch.randint(-32768, 32768, (nL * vs,), generator=gen, dtype=torch.int32).to(torch.int16)
    for t in (src_k, src_v):
        t[r0 * 64], t[r0 * 64 + 1], t[r0], t[r0 + 1] = 0x7FC0, 0x7C00, 0x7F81, 0x7E00
    sk, sv = src_k.cuda(), src_v.cuda()
    sk0, sv0 = sk.clone(), sv.clone()
    dk = torch.full((nL * kd,), _i16(SENT16), dtype=torch.int16, device="cuda")
    dv = torch.full((nL * vd,), _i16(SENT16), dtype=torch.int16, device="cuda")
    L.call("showo_kv_copy_rows", L.ptr(sk), L.ptr(sv), cap_src, ks, vs, L.ptr(dk), L.ptr(dv), cap_dst, kd, vd, nL, nH, r0, r1, base, L.stream())
    torch.cuda.synchronize()
    want_k = torch.full((nL * kd,), _i16(SENT16), dtype=torch.int16)
    want_v = torch.full((nL * vd,), _i16(SENT16), dtype=torch.int16)
    Z = (r1 - base + 63) // 64 * 64
    for li in range(nL):
        a = src_k[li * ks: li * ks + nH * cap_src * 64].reshape(nH, cap_src, 64)
        want_k[li * kd: li * kd + nH * cap_dst * 64].reshape(nH, cap_dst, 64)[:, r0 - base:r1 - base] = a[:, r0:r1]
        b = src_v[li * vs: li * vs + nH * 64 * cap_src].reshape(nH * 64, cap_src)
        w = want_v[li * vd: li * vd + nH * 64 * cap_dst].reshape(nH * 64, cap_dst)
        w[:, r0 - base:r1 - base] = b[:, r0:r1]
        w[:, r1 - base:Z] = 0
    assert torch.equal(dk.cpu(), want_k), ("K", r0, n)
    assert torch.equal(dv.cpu(), want_v), ("V^T", r0, n)
    assert torch.equal(sk, sk0) and torch.equal(sv, sv0)
    lib = L.load()
    args = lambda cs, cd, a, b, bs: (L.ptr(sk), L.ptr(sv), cs, ks, vs, L.ptr(dk), L.ptr(dv), cd, kd, vd, nL, nH, a, b, bs, L.stream())
    assert lib.showo_kv_copy_rows(*args(cap_src, cap_dst, r0, cap_src + 1, base)) == 5   # beyond the source
    assert lib.showo_kv_copy_rows(*args(cap_src, 64, 64, 130, 64)) == 5                  # beyond the destination
    assert lib.showo_kv_copy_rows(*args(cap_src, cap_dst, r0, r1, 32)) == 1              # base is no multiple of 64
    assert lib.showo_kv_copy_rows(*args(cap_src, cap_dst, r0, r0, base)) == 1            # empty range
