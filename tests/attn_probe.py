"""Attention test inputs in which single keys matter, an fp64 reference and a derived error bound (CPU).

With i.i.d. N(0, 1) data no key matters: dropping one of ctx keys, or reading one key too many, moves an
attention output by about 1 / ctx, far below any bf16 tolerance. The inputs built here make such an
error an O(1) error:

* **Probe keys.** Every (row, query head) has one hot key j*: the cache row K[j*] equals that head's bf16
  q, so its score is |q|^2 / sqrt(128) ~ 11.3 against N(0, 1) for the other keys and j* carries most of the
  softmax weight. The heads of a GQA group share K, so each gets its own j*. The hot keys cycle over the
  edges of the kernels' key partitions (edge_keys); `rnd` selects the next stretch of the cycle, so a few
  rounds visit every edge.
* **Poison tail.** Every cache position ctx .. Smax-1 holds K = bf16(4 * sum of the group's q) and V = 1000:
  its score exceeds every real score of every head by at least 10 (asserted), so one over-read key takes
  the whole softmax weight and the output jumps to ~1000. V stays finite: the kernels multiply the masked
  part of a loaded slice by p = 0, so NaN / Inf beyond the context are outside their contract.

**Reference and bound.** ref = the softmax-weighted sum over the visible keys in fp64. The kernels keep the
scores, the running max and l in fp32, round p to bf16 for the P.V MFMA and the normalised output to bf16.
A bf16 rounding moves a value by at most half an ulp of an 8-bit significand, 2^-8 of the value (just above a
power of two; 2^-9 just below the next): rounding p perturbs the numerator by at most 2^-8 * sum_j p_j |v_j|,
rounding the output by at most 2^-8 * |out|; the fp32 terms (scores, exp, l, the accumulation, the merge of
waves and splits) are orders of magnitude smaller and have the 1e-5. The elementwise bound is the sum:
    bound = 2^-8 * (sum_j p_j |v_j| + |ref|) + 1e-5
and a result passes when max(|out - ref| / bound) <= 1 (i.i.d. data sit near 0.49; one dominant term just
above a power of two comes to 0.9). emulate() restates the kernel arithmetic on the
CPU (fp32 scores and l, bf16 p, bf16 output) and takes the set of visible keys as an argument, which is how
tests/test_attn_probe_cpu.py shows what a masking or partition error does to this ratio.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import torch

HD = 128
AT_KB = 128                     # keys per workgroup iteration of k_attn_decode (4 waves x 32)
SCALE = 1.0 / HD ** 0.5
POISON_V = 1000.0
POISON_MARGIN = 10.0
P_HOT_MIN = 0.5


# ---------------------------------------------------------------------------- the kernels' key partitions
def block_split_keys(ctx: int, nsplit: int, split: int) -> range:
    """k_attn_decode: split `split` of nsplit owns the contiguous 128-key blocks
    [split * nkb / nsplit, (split + 1) * nkb / nsplit) of the nkb = ceil(ctx / 128) blocks."""
    nkb = (ctx + AT_KB - 1) // AT_KB
    kb0, kb1 = split * nkb // nsplit, (split + 1) * nkb // nsplit
    return range(kb0 * AT_KB, min(kb1 * AT_KB, ctx))


def slice_split_keys(ctx: int, nsplit: int, split: int, wave: int | None = None) -> list[int]:
    """k_attn_decode_qs: wave w of split `split` owns the 32-key slices split * 4 + w + j * 4 * nsplit."""
    nsl = (ctx + 31) // 32
    keys = []
    for w in (range(4) if wave is None else (wave,)):
        for s in range(split * 4 + w, nsl, 4 * nsplit):
            keys.extend(range(s * 32, min(s * 32 + 32, ctx)))
    return sorted(keys)


def wave_slice_keys(ctx: int, block: int, wave: int) -> range:
    """k_attn_decode: the 32-key slice of wave `wave` in 128-key block `block`."""
    lo = block * AT_KB + 32 * wave
    return range(lo, max(lo, min(lo + 32, ctx)))


def edge_keys(ctx: int, block_splits=(), slice_splits=()) -> list[int]:
    """The keys at which the decode kernels' masks and partitions begin or end, within 0 <= j < ctx."""
    e = {0, 31, 32, 127, 128, ctx - 1, ctx - 2, ctx // 2}
    e.add(((ctx - 1) // 32) * 32)                               # first key of the last 32-slice
    lb = ((ctx - 1) // AT_KB) * AT_KB
    e.update((lb, lb - 1))                                      # first key of the last 128-block, the key before
    for w in range(4):                                          # first key of each wave's last slice (kbw)
        b = (ctx - 32 * w + AT_KB - 1) // AT_KB - 1
        if ctx - 32 * w > 0:
            e.add(b * AT_KB + 32 * w)
    for ns in block_splits:
        for sp in range(ns):
            ks = block_split_keys(ctx, ns, sp)
            if len(ks):
                e.update((ks[0], ks[-1]))
    for ns in slice_splits:                                     # (per wave: a split's waves stride on their own)
        for sp in range(ns):
            for w in range(4):
                ks = slice_split_keys(ctx, ns, sp, wave=w)
                if ks:
                    e.update((ks[0], ks[-1]))
    return sorted(j for j in e if 0 <= j < ctx)


def n_rounds(edges, R, H, Hk, newest=False) -> int:
    """Rounds of decode_probe after which every edge key has been some head's hot key."""
    per = R * (H - Hk if newest else H)
    return max(1, -(-len(edges) // per))


# ---------------------------------------------------------------------------- reference, bound, emulation
def reference(q, k, v, visible):
    """q [B][T][128], k / v [B][J][128], visible bool broadcastable to [B][T][J] -> (ref, bound, p) in fp64:
    the softmax-weighted sum over the visible keys, the elementwise bound of the module docstring and the
    softmax weights."""
    if q.shape[0] > 64:                                         # (fp64 copies of a large cache: in pieces)
        vis = visible.expand(q.shape[0], q.shape[1], k.shape[1]) if visible.dim() == 3 else None
        parts = [reference(q[i:i + 64], k[i:i + 64], v[i:i + 64], visible if vis is None else vis[i:i + 64])
                 for i in range(0, q.shape[0], 64)]
        return tuple(torch.cat(x) for x in zip(*parts))
    qd, kd, vd = q.double(), k.double(), v.double()
    s = torch.einsum("btd,bjd->btj", qd, kd) * SCALE
    s = s.masked_fill(~visible.expand_as(s), -float("inf"))
    p = torch.softmax(s, dim=-1)
    ref = torch.einsum("btj,bjd->btd", p, vd)
    pabs = torch.einsum("btj,bjd->btd", p, vd.abs())
    return ref, 2.0 ** -8 * (pabs + ref.abs()) + 1e-5, p


def emulate(q, k, v, visible):
    """The kernels' arithmetic on the CPU over the keys `visible` (same shapes as reference): fp32 scores,
    max and l, p rounded to bf16 for P.V, fp32 accumulation, the normalised output rounded to bf16."""
    qf, kf, vf = q.float(), k.float(), v.float()
    s = torch.einsum("btd,bjd->btj", qf, kf) * SCALE
    s = s.masked_fill(~visible.expand_as(s), -float("inf"))
    m = s.max(dim=-1, keepdim=True).values
    p = torch.exp(s - m)
    l = p.sum(dim=-1, keepdim=True)
    o = torch.einsum("btj,bjd->btd", p.to(torch.bfloat16).float(), vf)
    return (o / l).to(torch.bfloat16)


def ratio(out, ref, bound) -> float:
    """max(|out - ref| / bound); a NaN or Inf in `out` counts as infinitely wrong."""
    o = out.double().reshape(ref.shape)
    if not bool(torch.isfinite(o).all()):
        return float("inf")
    return float(((o - ref).abs() / bound).max())


def merge_partials(work, R, H, Hk, nsplit):
    """The (m, l, O) partials [R][Hk][nsplit][8 + 4 * 128] of the *_part entries merged in fp64 -> the
    normalised attention [R][H][128] (the 4 head slots of a group beyond H / Hk are dropped)."""
    wk = work.detach().cpu().reshape(R, Hk, nsplit, 8 + 4 * HD).double()
    m, l, o = wk[..., :4], wk[..., 4:8], wk[..., 8:].reshape(R, Hk, nsplit, 4, HD)
    M = m.max(dim=2, keepdim=True).values
    c = torch.where(m == -float("inf"), torch.zeros_like(m), torch.exp(m - M))
    G = H // Hk
    att = (o * c[..., None]).sum(2)[:, :, :G] / (l * c).sum(2)[:, :, :G, None]
    return att.reshape(R, H, HD)


# ---------------------------------------------------------------------------- decode probes
@dataclass
class DecodeProbe:
    R: int
    H: int
    Hk: int
    ctx: int
    smax: int
    q: torch.Tensor                   # [R][H][128] bf16
    k: torch.Tensor                   # [R][Hk][smax][128] bf16: the cache the reference sees
    v: torch.Tensor
    k_in: torch.Tensor                # the cache handed to the kernel (differs from k / v at key ctx - 1 when
    v_in: torch.Tensor                # the kernel itself supplies the newest key)
    hot: torch.Tensor                 # [R][H] int64, -1: no probe (fewer edge keys than heads in the group)
    ref: torch.Tensor = field(default=None)      # [R][H][128] fp64
    bound: torch.Tensor = field(default=None)
    p: torch.Tensor = field(default=None)        # [R][H][smax] fp64
    quant: dict = field(default=None)            # FP8: kq, ks, vq, vs bytes of k_in / v_in, *_ref of k / v

    def _bh(self, x):                 # cache [R][Hk][smax][128] -> one batch per (row, kv head)
        return x.reshape(self.R * self.Hk, self.smax, HD)

    def _qb(self):                    # the group's heads are the batch's queries
        return self.q.reshape(self.R * self.Hk, self.H // self.Hk, HD)

    def visible(self, keys=None):
        """[smax] bool: the keys < ctx, or exactly `keys`."""
        vis = torch.zeros(self.smax, dtype=torch.bool)
        if keys is None:
            vis[:self.ctx] = True
        else:
            vis[list(keys)] = True
        return vis

    def emulate(self, visible=None):
        vis = self.visible() if visible is None else visible
        return emulate(self._qb(), self._bh(self.k), self._bh(self.v), vis).reshape(self.R, self.H, HD)

    def ratio(self, out) -> float:
        """out: anything of R * H * 128 elements (a kernel's [R][H * 128] bf16 output)."""
        return ratio(out.detach().cpu().reshape(self.R, self.H, HD), self.ref, self.bound)

    def finish(self):
        """The reference and the two preconditions: every probe's hot key holds at least half the softmax
        weight, and a poisoned key's score beats every real score of every head by POISON_MARGIN."""
        R, H, ctx = self.R, self.H, self.ctx
        qb = self._qb()
        ref, bound, p = reference(qb, self._bh(self.k), self._bh(self.v), self.visible())
        self.ref, self.bound, self.p = ref.reshape(R, H, HD), bound.reshape(R, H, HD), p.reshape(R, H, self.smax)
        hot = self.hot.reshape(-1)
        ph = self.p.reshape(R * H, -1).gather(1, hot.clamp(min=0)[:, None])[:, 0]
        ph = torch.where(hot >= 0, ph, torch.ones_like(ph))
        assert float(ph.min()) >= P_HOT_MIN, f"a hot key holds only p = {float(ph.min()):.3f} at ctx {ctx}"
        if self.smax > ctx:
            s = torch.einsum("btd,bjd->btj", qb.double(), self._bh(self.k).double()) * SCALE
            margin = s[..., ctx:].min(dim=-1).values - s[..., :ctx].max(dim=-1).values
            assert float(margin.min()) >= POISON_MARGIN, f"poison margin {float(margin.min()):.2f} at ctx {ctx}"
            assert bool(torch.isfinite(self._bh(self.v).float()).all())
        return self


def _poison_margin(q, R, H, Hk):
    """Per (row, group): the smallest (poisoned score - hot score) over the group's heads, from q alone
    (the hot score |q|^2 / sqrt(128) is by far a head's largest real score)."""
    G = H // Hk
    qg = q.float().reshape(R, Hk, G, HD)
    pz = (4 * qg.sum(2)).to(torch.bfloat16).float()
    sp = torch.einsum("rghd,rgd->rgh", qg, pz) * SCALE
    sh = (qg * qg).sum(-1) * SCALE
    return (sp - sh).min(dim=2).values


def _bad_groups(q, R, H, Hk, ctx, slack):
    """[R][Hk] bool: groups whose q would miss a precondition -- the poison margin (+ slack for the real scores'
    N(0, 1) maximum), or a hot score |q|^2 / sqrt(128) too small to outweigh ctx keys of score N(0, 1), whose
    exp sums to ~1.65 ctx (p(j*) >= 2/3 asked for here, >= 0.5 asserted on the cache)."""
    import math
    sh = (q.float().reshape(R, Hk, H // Hk, HD) ** 2).sum(-1) * SCALE
    return (_poison_margin(q, R, H, Hk) < POISON_MARGIN + slack) | (sh.min(dim=2).values < math.log(3.3 * ctx))


def draw_q(R, H, Hk, g, ctx=1):
    """q [R][H][128] ~ bf16(N(0, 1)); a group that would miss a precondition is redrawn (the hot score is
    11.3 +- 1.4 and needs 9.2 at ctx 2999; the cross terms between a group's q are N(0, 1) each)."""
    q = torch.randn(R, H, HD, generator=g).to(torch.bfloat16)
    for _ in range(64):
        bad = _bad_groups(q, R, H, Hk, ctx, 4.0)
        if not bool(bad.any()):
            return q
        new = torch.randn(R, H, HD, generator=g).to(torch.bfloat16).reshape(R, Hk, H // Hk, HD)
        qv = q.reshape(R, Hk, H // Hk, HD)
        qv[bad] = new[bad]
    raise AssertionError("no q with the preconditions")


def decode_probe(R, H, Hk, ctx, smax, edges, seed, rnd=0, q=None, newest=None, fp8=False) -> DecodeProbe:
    """Probe cache for one decode-attention launch.

    q: the queries [R][H][128] bf16 (drawn here when None).
    newest: (k_new, v_new) [R][Hk][128] bf16 -- the fused entries compute key ctx - 1 themselves: the
        reference sees it at ctx - 1, the input cache holds poison there (so a key that is not patched in
        ruins the output), the first head of every group has it as its hot key (the caller made that
        head's q equal to k_new) and the other heads' hot keys stay below ctx - 1.
    fp8: the cache is quantised with kvlayout.quantize_kv_e4m3 and the reference taken on the dequantised
        values (power-of-two scales: the kernel's numbers are exactly those, so the bound is unchanged).
    """
    from zonos_amd import kvlayout as kl
    assert 1 <= ctx <= smax and H % Hk == 0
    G = H // Hk
    g = torch.Generator().manual_seed(seed)
    if q is None:
        q = draw_q(R, H, Hk, g, ctx)
    q = q.reshape(R, H, HD).cpu()
    k = torch.randn(R, Hk, smax, HD, generator=g).to(torch.bfloat16)
    v = torch.randn(R, Hk, smax, HD, generator=g).to(torch.bfloat16)
    lim = ctx - 1 if newest is not None else ctx
    cyc = [j for j in edges if j < lim]
    hot = torch.full((R, H), -1, dtype=torch.int64)
    n = rnd * R * H
    for r in range(R):
        for h in range(H):
            if newest is not None and h % G == 0:
                hot[r, h] = ctx - 1
                continue
            if cyc:
                j = cyc[n % len(cyc)]
                n += 1
                if not any(int(hot[r, h2]) == j for h2 in range(h - h % G, h)):   # one owner per cache row
                    hot[r, h] = j
                    k[r, h // G, j] = q[r, h]
    poison = (4 * q.float().reshape(R, Hk, G, HD).sum(2)).to(torch.bfloat16)
    k[:, :, ctx:] = poison[:, :, None]
    v[:, :, ctx:] = POISON_V
    k_in, v_in = k, v
    if newest is not None:
        k_in, v_in = k.clone(), v.clone()
        k_in[:, :, ctx - 1] = poison
        v_in[:, :, ctx - 1] = POISON_V
        k[:, :, ctx - 1], v[:, :, ctx - 1] = newest[0].cpu(), newest[1].cpu()
    quant = None
    if fp8:
        (kq, ks), (vq, vs) = kl.quantize_kv_e4m3(k_in), kl.quantize_kv_e4m3(v_in)
        (kqr, ksr), (vqr, vsr) = kl.quantize_kv_e4m3(k), kl.quantize_kv_e4m3(v)
        quant = dict(kq=kq, ks=ks, vq=vq, vs=vs, kq_ref=kqr, ks_ref=ksr, vq_ref=vqr, vs_ref=vsr)
        k_in, v_in = kl.dequantize_kv_e4m3(kq, ks), kl.dequantize_kv_e4m3(vq, vs)
        k, v = kl.dequantize_kv_e4m3(kqr, ksr), kl.dequantize_kv_e4m3(vqr, vsr)
    return DecodeProbe(R, H, Hk, ctx, smax, q, k, v, k_in, v_in, hot, quant=quant).finish()


def fused_part(R, H, Hk, gs, seed, ctx=1):
    """in_proj split-K slabs [gs][R][(H + 2 Hk) * 128] fp32 for the fused entries: N(0, 1 / gs) per slab (the
    reduced q, k, v are N(0, 1)), and in every slab the Q columns of the first head of each group equal the
    group's K columns, so that head's q (after the same RoPE) is the newest key bit for bit. Groups whose q
    would miss a precondition are redrawn (RoPE rotates all heads alike: it keeps their dot products)."""
    G = H // Hk
    g = torch.Generator().manual_seed(seed)
    N = (H + 2 * Hk) * HD
    part = torch.randn(gs, R, N, generator=g) / gs ** 0.5
    for _ in range(64):
        pq = part[:, :, :H * HD].reshape(gs, R, Hk, G, HD)
        pq[:, :, :, 0] = part[:, :, H * HD:(H + Hk) * HD].reshape(gs, R, Hk, HD)
        qsum = part[:, :, :H * HD].sum(0).to(torch.bfloat16)
        bad = _bad_groups(qsum.reshape(R, H, HD), R, H, Hk, ctx, 6.0)
        if not bool(bad.any()):
            return part
        new = torch.randn(gs, R, N, generator=g) / gs ** 0.5
        for r, gi in bad.nonzero().tolist():
            part[:, r, gi * G * HD:(gi + 1) * G * HD] = new[:, r, gi * G * HD:(gi + 1) * G * HD]
            part[:, r, (H + gi) * HD:(H + gi + 1) * HD] = new[:, r, (H + gi) * HD:(H + gi + 1) * HD]
    raise AssertionError("no slabs with the poison margin")


# ---------------------------------------------------------------------------- prefill probes (causal)
@dataclass
class PrefillProbe:
    R: int
    S: int
    H: int
    Hk: int
    smax: int
    q: torch.Tensor                   # [R][S][H][128] bf16
    k: torch.Tensor                   # [R][Hk][smax][128] bf16
    v: torch.Tensor
    future: list                      # the t' whose key t' + 1 is future-hot for (t', a diagonal head of each group)
    ref: torch.Tensor = field(default=None)      # [R][S][H][128] fp64
    bound: torch.Tensor = field(default=None)

    def _args(self):
        G = self.H // self.Hk
        qb = self.q.permute(0, 2, 1, 3).reshape(self.R * self.H, self.S, HD)
        kb = self.k.repeat_interleave(G, dim=1).reshape(self.R * self.H, self.smax, HD)
        vb = self.v.repeat_interleave(G, dim=1).reshape(self.R * self.H, self.smax, HD)
        return qb, kb, vb

    def visible(self, shift=0):
        """[S][smax] bool: key <= t + shift."""
        t = torch.arange(self.S)[:, None]
        return torch.arange(self.smax)[None, :] <= t + shift

    def _unbh(self, x):
        return x.reshape(self.R, self.H, self.S, HD).permute(0, 2, 1, 3)

    def emulate(self, shift=0):
        return self._unbh(emulate(*self._args(), self.visible(shift)))

    def ratio(self, out) -> float:
        """out: [R * S][H * 128] (the kernel's layout) or [R][S][H][128]."""
        return ratio(out.detach().cpu().reshape(self.R, self.S, self.H, HD), self.ref, self.bound)


PREFILL_S = [1, 15, 16, 17, 33, 64, 65, 129]


def prefill_future(S):
    """The t' of the future-hot keys: the last query of a 16-query wave, of a 32-key slice, of a 64-query
    workgroup, and the one before the last."""
    return sorted({t for t in (15, 31, 63, S - 2) if 0 < t and t + 1 < S})


def _prefill_kind(h, t, G):
    """0, 1: the hot key of (query t, head h) is t; 2: key 0; 3: the first key of t's 32-slice. Rotated by t,
    and spread so that a group of 2 or 4 heads always has a diagonal head."""
    return ((h % G) * max(1, 4 // G) + t) % 4


def _future_head(t, G):
    """The head of a group whose q at t' = t becomes the future-hot key: a diagonal one (its q = K[t'] is no
    other query's)."""
    return next(h for h in range(G) if _prefill_kind(h, t, G) < 2)


def prefill_probe(R, S, H, Hk, smax, seed, future=()) -> PrefillProbe:
    """Causal probes. The cache keys are N(0, 1); every query is a copy of one of them, its hot key: for
    query t half the heads take key t (the diagonal), the others key 0 or the first key of t's 32-slice
    (_prefill_kind: rotated by t, so every head has every kind). Every probe's hot key holds p >= 0.5
    (asserted before the future-hot keys go in). The tail S .. smax-1 is poisoned as for decode, with the
    group sum of the last query (the one next to it).
    future: for each t' (t' + 1 < S) key t' + 1 becomes K = bf16(4 q[t'][a diagonal head of the group]), V = 1000:
    a mask that lets query t' see one key too many ruins it (asserted: that score exceeds the query's
    largest visible score by POISON_MARGIN); the reference includes the key for the queries after t'."""
    assert 1 <= S <= smax and H % Hk == 0
    G = H // Hk
    g = torch.Generator().manual_seed(seed)
    k = torch.randn(R, Hk, smax, HD, generator=g).to(torch.bfloat16)
    v = torch.randn(R, Hk, smax, HD, generator=g).to(torch.bfloat16)
    q = torch.empty(R, S, H, HD, dtype=torch.bfloat16)
    hot = torch.empty(S, H, dtype=torch.int64)
    for t in range(S):
        for h in range(H):
            kind = _prefill_kind(h, t, G)
            hot[t, h] = t if kind < 2 else (0 if kind == 2 else (t // 32) * 32)
            q[:, t, h] = k[:, h // G, hot[t, h]]
    # (the last query's heads share vectors: each distinct one counts once, or the repeated one would
    # outweigh the others' own term)
    first = [h for h in range(G) if int(hot[S - 1, h]) not in [int(hot[S - 1, h2]) for h2 in range(h)]]
    poison = (4 * q[:, S - 1].float().reshape(R, Hk, G, HD)[:, :, first].sum(2)).to(torch.bfloat16)
    k[:, :, S:] = poison[:, :, None]
    v[:, :, S:] = POISON_V
    pp = PrefillProbe(R, S, H, Hk, smax, q, k, v, list(future))
    _, _, p = reference(*pp._args(), pp.visible())
    ph = p.reshape(R, H, S, smax).gather(3, hot.t()[None, :, :, None].expand(R, H, S, 1))
    assert float(ph.min()) >= P_HOT_MIN, f"a hot key holds only p = {float(ph.min()):.3f} at S {S}"
    for t in future:
        assert 0 < t and t + 1 < S          # (key 0 is the hot key of a quarter of all queries: not t' = 0)
        k[:, :, t + 1] = (4 * q[:, t, _future_head(t, G)::G].float()).to(torch.bfloat16)
        v[:, :, t + 1] = POISON_V
    qb, kb, vb = pp._args()
    s = torch.einsum("btd,bjd->btj", qb.double(), kb.double()).reshape(R, H, S, smax) * SCALE
    for t in list(future) + [S - 1]:
        if t + 1 < smax:
            hs = slice(_future_head(t, G), H, G) if t != S - 1 else slice(0, H)
            margin = s[:, hs, t, t + 1] - s[:, hs, t, :t + 1].max(dim=-1).values
            assert float(margin.min()) >= POISON_MARGIN, f"future / poison margin {float(margin.min()):.2f} at t {t}"
    ref, bound, _ = reference(qb, kb, vb, pp.visible())
    pp.ref, pp.bound = pp._unbh(ref), pp._unbh(bound)
    return pp
