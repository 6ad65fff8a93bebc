"""Mamba2 mixer test inputs in which one time step, one conv tap or one state element matters, an fp64
reference at the kernels' interface with an elementwise error bound, and an fp32 restatement with mutant
switches (CPU; zonos_amd/csrc/mamba.hip is what they describe).

A recurrence hides errors: an update that is wrong at one step has decayed by the end of the sequence, and with
D = 1 the skip term D*x dominates y. The cases built here keep such errors O(1) in a named output.

**Reference.** reference() computes, in fp64, what zk_mamba_prefill / zk_mamba_step / zk_gated_rmsnorm compute
from the in_proj output zx (fp32 [R][S][ncol], or its split-K slabs [gs][R][S][ncol]; the columns are
z | x B C | dt), the taps conv_w [conv_dim][4], conv_b, A, dt_bias, D, the norm weight and the initial conv and
SSM states.
The kernels' rounding points are stated as they occur:
  (1) every in_proj column is rounded to bf16 after the slab sum (col);
  (2) xc = bf16(silu(conv_b + sum_k w[k] * in[t-3+k])), the conv state is the last four bf16 inputs (exact);
  (3) the SSM state h is stored as bf16 after the steps in `round_at` -- once, after the last step, by a
      prefill (fp32 registers in between), after every step by the decode kernel (round_points());
  (4) y = bf16(C.h + D*x) before the fp32 gate g = y * silu(z);
  (5) out = bf16(g * rsqrt(mean(g^2) + eps) * w).

**Bound.** Beside every reference value an upper bound of |device - reference| is carried. With u =
F32_TERM * 2^-24, the named fp32 term (rounding of one fp32 operation, a transcendental's error, the order of
a sum; the constant is chosen from measurements, below):
  conv   : e_pre = u * (1.1 * (|b| + sum|w in|) + |silu|)          (silu' <= 1.1)
  dt     : e_dt = u * dt;   dA = exp(dt A): e_dA = dA * u * (1 + 2 |dt A|)
  state  : e_h(t) = e_h(t-1) * dA + (|h(t-1)| + e_h(t-1)) * e_dA + e_inj + u * |h(t)|,
           e_inj = e_B dt |x| + |B| dt e_x + e_B dt e_x + 3 u |B dt x|   (e_x, e_B, e_C: the errors of xc)
  y      : e_y = sum_n (|C| e_h + e_C (|h| + e_h)) + u * sum_n |C h| + |D| e_x + u |D x|
  gate   : e_g = e_y |silu(z)| + 3 u |g|
  norm   : e_ms = mean(2 |g| e_g + e_g^2) + u ms;  rstd_hi = rsqrt(max(ms - e_ms, 0) + eps);
           e_pre = (e_g rstd_hi + |g| (rstd_hi - rstd + 2 u rstd)) |w| + 2 u |pre|
At a bf16 rounding point a value known to e_pre comes out either identical -- when e_pre is smaller than the
distance of the fp64 value from the nearest midpoint of two bf16 neighbours, no admissible input rounds the
other way -- or off by at most e_pre plus one whole ulp (rounding is monotone: |rn(a) - rn(b)| <= |a - b| +
ulp). round_err() applies exactly that, so a one-ulp flip is allowed at every rounding point at which the
device's expf / log1pf / summation order can produce one, and only there. Passing xc= (the device's own conv
output, checked separately to be within one ulp of the reference's) removes e_x, e_B and e_C.
A result passes when ratio() = max(|got - ref| / bound) <= 1.

**The fp32 term.** F32_TERM = 4, chosen from measurements with the bound evaluated at smaller terms
(f32_term=): the fp32 restatement emulate() stays within the bound with half of it (2; it does not with 1;
asserted in tests/test_mamba_probe_cpu.py), and so do the MI355X kernels in every GPU test (2, a margin of 2 x
where 1.5 x is asked for, because the device's expf / log1pf and reduction order differ from torch's);
profiles/mamba_probe_tests.txt has the figures per family and geometry. Because a permitted flip is one ulp
against a bound of one ulp plus little, the largest ratio of a clean result is 1.000 wherever a flip occurs:
the margin shows in the term that is needed, not in the ratio. sharp=False gives the loose bound (a flip allowed
at every rounding point) for finite figures to print; it is no criterion.

**Cases** (make_case(); check_properties() asserts what is claimed). R = 3 rows, nh = 4 heads, the three
instantiated (headdim, d_state) pairs, S in LENGTHS. All zx values are bf16 values on a 2^-10 grid, so slabs()
can split them into gs fp32 slabs whose sum, in the kernels' order, is exact.
* heads: 0 slow (A = -2^-9: dA within 5e-3 of 1, an error at step 0 or at a chunk boundary is still there in
  the final state; D = 0, so y is the state term alone), 1 fast (A = -16, dt in 2.5 .. 4.5: forgets within a
  step; D = -2.5),
  2 on the softplus threshold (dt_bias = 20, raw dt = +-(3..4) alternating over rows and time; D = 0),
  3 medium (D = +1.75). A, dt_bias, D are distinct per head.
* taps: distinct and non-symmetric per channel; the B / C channels' taps are dominated by the newest input
  (w3 about 1, the others a few percent), which is what lets a row choose its B_t and C_t.
* the probe row R-1: its B and C inputs are -24 everywhere and +6 on one hot channel, so B_t and C_t are one-hot
  over d_state to within 1e-5. The hot index of B cycles over hot_indices() (the edges of the kernels'
  per-thread runs of EPT state elements, of the 8-element packs and of the grouped kernel's 16-lane x
  8-channel pieces), and C_t reads back what B wrote at step t - t % 3. One dropped, duplicated or misplaced
  state element is an O(1) error in yz[R-1][t][head * headdim + p] (drop_target() names one).
* impulses of 6.0 in x at t in {0, 1, 2, 3, 15, 16, 17, S-4 .. S-1} on a channel that depends on (t, row);
  everything else is i.i.d., so every row, head and channel carries different data (z included).

emulate() restates the kernels in fp32 (torch, CPU) with their buffers: the conv and SSM states double-buffered
by position parity, prefill(S0) writing the parity-(S0 & 1) buffers, the steps S0 .. S-1 reading (t & 1) and
writing the other. `mutant=` switches one deliberate error on (MUTANTS); tests/test_mamba_probe_cpu.py shows
that each of them exceeds the bound on the cases aimed at it.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

F32_TERM = 4.0                                 # the fp32 term in units of 2^-24 (module docstring)
SILU_LIP = 1.1
GEOMS = ((32, 64), (64, 64), (64, 128))        # the instantiated (headdim, d_state)
NH, ROWS = 4, 3
LENGTHS = (1, 2, 3, 4, 5, 15, 16, 17, 33)
THREADS, CHUNK = 256, 16                       # mamba.hip: MB_THREADS, the scan's LDS chunk
NORM_EPS = 1e-5

MUTANTS = ("taps_swapped", "taps_shifted", "no_zero_pad", "conv_state_off_by_one", "chunk_reset", "no_carry",
           "parity_wrong", "drop_element", "b_prev", "bc_exchanged", "dt_bias_neighbour", "a_neighbour",
           "softplus_wrong_threshold", "threshold_branch_clamped", "no_d", "z_neighbour", "slab_last_dropped",
           "y_not_rounded")


# ---------------------------------------------------------------------------- bf16 in fp64
def bf(x):
    """x rounded to bf16 (nearest, ties to even), in fp64."""
    m, e = np.frexp(np.asarray(x, dtype=np.float64))
    return np.ldexp(np.round(np.ldexp(m, 8)), e - 8)


def ulp(x):
    """The spacing of bf16 values at |x|."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    _, e = np.frexp(x)
    return np.where(x > 0, np.ldexp(1.0, e - 8), 0.0)


def round_err(pre, err, sharp=True):
    """(bf16(pre), bound of |bf16(v) - bf16(pre)| over |v - pre| <= err): 0 where no such v rounds the other
    way, else err plus one ulp. The distance to the nearest midpoint is taken on the safe side at a power of
    two (the midpoint below it is a quarter of the upper spacing away). sharp=False: err plus one ulp
    everywhere (the loose bound, for finite figures only)."""
    r, u = bf(pre), ulp(pre)
    off = np.abs(pre - r)
    dist = np.minimum(0.5 * u - off, 0.25 * u + off)
    return r, np.where((err < dist) & sharp, 0.0, err + ulp(np.abs(pre) + err))


def ratio(got, ref, bound) -> float:
    """max |got - ref| / bound (0 where got == ref, inf where they differ and the bound is 0)."""
    d = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(d == 0, 0.0, d / bound)
    return float(q.max()) if q.size else 0.0


def round_points(S, S0):
    """The steps after which the SSM state is stored as bf16: prefill(S0), then the steps S0 .. S-1."""
    return frozenset(t for t in ([S0 - 1] + list(range(S0, S))) if t >= 0)


# ---------------------------------------------------------------------------- parameters
@dataclass
class Params:
    conv_w: np.ndarray            # fp32 [conv_dim][4]
    conv_b: np.ndarray            # fp32 [conv_dim]
    A: np.ndarray                 # fp32 [nh] (negative)
    dt_bias: np.ndarray           # fp32 [nh]
    D: np.ndarray                 # fp32 [nh]
    norm_w: np.ndarray            # fp32 [d_inner]

    def dims(self, ncol):
        """(d_inner, d_state, nh, headdim, conv_dim) from the in_proj width."""
        nh, cd = self.A.shape[0], self.conv_w.shape[0]
        di = ncol - nh - cd
        ds = (cd - di) // 2
        assert di > 0 and di % nh == 0 and di + 2 * ds == cd, (ncol, nh, cd)
        return di, ds, nh, di // nh, cd


@dataclass
class Ref:
    xc: np.ndarray                # [R][S][conv_dim]; e_xc its bound (0 where xc was given)
    e_xc: np.ndarray
    conv: np.ndarray              # [R][S][conv_dim][4]: the conv state after every step (exact)
    ssm: np.ndarray               # [R][nh][hp][ds] after the last step, as stored; e_ssm
    e_ssm: np.ndarray
    yz: np.ndarray                # [R][S][d_inner]; e_yz
    e_yz: np.ndarray
    out: np.ndarray               # [R][S][d_inner] gated RMSNorm; e_out
    e_out: np.ndarray


def _softplus_thr(v):
    return np.where(v <= 20.0, np.log1p(np.exp(np.minimum(v, 20.0))), v)


def norm_reference(g, e_g, w, eps=NORM_EPS, f32_term=F32_TERM, sharp=True):
    """RMSNormGated(norm_before_gate=False) over the last axis of g (known to e_g) -> (out, bound)."""
    u = f32_term * 2.0 ** -24
    ms = np.mean(g * g, axis=-1, keepdims=True)
    e_ms = np.mean(2 * np.abs(g) * e_g + e_g * e_g, axis=-1, keepdims=True) + u * ms
    rstd = 1.0 / np.sqrt(ms + eps)
    rstd_hi = 1.0 / np.sqrt(np.maximum(ms - e_ms, 0.0) + eps)
    pre = g * rstd * w
    e_pre = (e_g * rstd_hi + np.abs(g) * (rstd_hi - rstd + 2 * u * rstd)) * np.abs(w) + 2 * u * np.abs(pre)
    return round_err(pre, e_pre, sharp)


def reference(zx, P: Params, conv0=None, ssm0=None, round_at=frozenset(), xc=None, f32_term=F32_TERM,
              sharp=True) -> Ref:
    """The fp64 reference and its bound (module docstring). conv0 [R][conv_dim][4] and ssm0 [R][nh][hp][ds] hold
    bf16 values (None: zeros); xc [R][S][conv_dim]: take these conv outputs instead of the reference's own;
    f32_term: the fp32 term the bound is evaluated with; sharp=False: the loose bound (round_err)."""
    u = f32_term * 2.0 ** -24
    zx = np.asarray(zx, dtype=np.float64)
    if zx.ndim == 4:
        zx = zx.sum(0)
    col = bf(zx)                                                        # (1)
    R, S, ncol = col.shape
    di, ds, nh, hp, cd = P.dims(ncol)
    z, xBC, dtc = col[..., :di], col[..., di:di + cd], col[..., di + cd:]
    w, b = P.conv_w.astype(np.float64), P.conv_b.astype(np.float64)
    A, dtb, Dv = (a.astype(np.float64) for a in (P.A, P.dt_bias, P.D))
    conv0 = np.zeros((R, cd, 4)) if conv0 is None else np.asarray(conv0, dtype=np.float64)
    hist = np.concatenate([conv0.transpose(0, 2, 1)[:, 1:], xBC], axis=1)         # row j: the input j - 3
    acc = np.broadcast_to(b, (R, S, cd)).copy()
    mag = np.abs(acc)
    for k in range(4):
        acc += w[:, k] * hist[:, k:k + S]
        mag += np.abs(w[:, k] * hist[:, k:k + S])
    pre = acc / (1.0 + np.exp(-acc))
    xc_ref, e_xc = round_err(pre, u * (SILU_LIP * mag + np.abs(pre)), sharp)   # (2)
    if xc is not None:
        xc_ref, e_xc = np.asarray(xc, dtype=np.float64), np.zeros_like(e_xc)
    conv = np.stack([hist[:, t:t + 4].transpose(0, 2, 1) for t in range(S)], axis=1)
    h = np.zeros((R, nh, hp, ds)) if ssm0 is None else np.asarray(ssm0, dtype=np.float64).copy()
    e_h = np.zeros_like(h)
    yz, e_yz = np.zeros((R, S, di)), np.zeros((R, S, di))
    for t in range(S):
        x, e_x = (a[:, t, :di].reshape(R, nh, hp, 1) for a in (xc_ref, e_xc))
        B, e_B = (a[:, t, di:di + ds].reshape(R, 1, 1, ds) for a in (xc_ref, e_xc))
        C, e_C = (a[:, t, di + ds:].reshape(R, 1, 1, ds) for a in (xc_ref, e_xc))
        dt = _softplus_thr(dtc[:, t] + dtb)                             # [R][nh]
        a = dt * A
        dA = np.exp(a)
        e_dA = (dA * u * (1 + 2 * np.abs(a)))[:, :, None, None]
        dt, dA = dt[:, :, None, None], dA[:, :, None, None]
        inj = B * dt * x
        e_inj = e_B * dt * np.abs(x) + np.abs(B) * dt * e_x + e_B * dt * e_x + 3 * u * np.abs(inj)
        hn = h * dA + inj
        e_h = e_h * dA + (np.abs(h) + e_h) * e_dA + e_inj + u * np.abs(hn)
        h = hn
        Dh = Dv[None, :, None]
        ypre = (C * h).sum(-1) + Dh * x[..., 0]
        e_y = (np.abs(C) * e_h + e_C * (np.abs(h) + e_h)).sum(-1) + u * np.abs(C * h).sum(-1) \
            + np.abs(Dh) * e_x[..., 0] + u * np.abs(Dh * x[..., 0])
        y, e_y = round_err(ypre, e_y, sharp)                              # (4)
        zz = z[:, t].reshape(R, nh, hp)
        sz = zz / (1.0 + np.exp(-zz))
        g = y * sz
        yz[:, t] = g.reshape(R, di)
        e_yz[:, t] = (e_y * np.abs(sz) + 3 * u * np.abs(g)).reshape(R, di)
        if t in round_at:
            h, e_h = round_err(h, e_h, sharp)                           # (3)
    out, e_out = norm_reference(yz, e_yz, P.norm_w.astype(np.float64), f32_term=f32_term, sharp=sharp)   # (5)
    return Ref(xc_ref, e_xc, conv, h, e_h, yz, e_yz, out, e_out)


# ---------------------------------------------------------------------------- the fp32 restatement
def _rb(x):
    return x.to(torch.bfloat16).float()


def emulate(zx, P: Params, S0, conv0=None, ssm0=None, mutant=None, arg=None):
    """The kernels' arithmetic in fp32: zk_mamba_prefill over the steps 0 .. S0-1 (from zero states), then
    zk_mamba_step at the positions S0 .. S-1 (S0 = 0: from conv0 / ssm0 in the parity-0 buffers), then
    zk_gated_rmsnorm. -> dict(xc, conv (the state written after every step; prefill steps: the state a
    prefill of that length writes), ssm (the buffer the step at position S reads), yz, out), numpy.
    arg of drop_element: (row, head, p, n, t)."""
    assert mutant is None or mutant in MUTANTS, mutant
    f = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32))
    zx = f(zx)
    if zx.ndim == 4:                                                    # slab_col: v0 + v1 + ... in order
        n = zx.shape[0] - (1 if mutant == "slab_last_dropped" else 0)
        a = zx[0].clone()
        for s in range(1, n):
            a = a + zx[s]
        zx = a
    col = _rb(zx)
    R, S, ncol = col.shape
    di, ds, nh, hp, cd = P.dims(ncol)
    z, xBC, dtc = col[..., :di], col[..., di:di + cd], col[..., di + cd:]
    w, b, A, dtb, Dv, nw = (f(a) for a in (P.conv_w, P.conv_b, P.A, P.dt_bias, P.D, P.norm_w))
    if mutant == "taps_swapped":
        w = w.flip(1)
    if mutant == "a_neighbour":
        A = A.roll(-1)
    if mutant == "dt_bias_neighbour":
        dtb = dtb.roll(-1)
    if mutant == "z_neighbour":
        z = z.reshape(R, S, nh, hp).roll(-1, 2).reshape(R, S, di)
    zero_in = torch.zeros(R, cd)
    conv_buf = [torch.zeros(R, cd, 4), torch.zeros(R, cd, 4)]
    ssm_buf = [torch.zeros(R, nh, hp, ds), torch.zeros(R, nh, hp, ds)]
    if conv0 is not None:
        conv_buf[0] = f(conv0).clone()
    if ssm0 is not None:
        ssm_buf[0] = f(ssm0).clone()

    def inp(v, taps=False):                  # the prefill's zero-padded history
        if mutant == "no_zero_pad" and taps:
            v = max(v, 0)
        return xBC[:, v] if 0 <= v < S0 else zero_in

    h = torch.zeros(R, nh, hp, ds)           # the scan's registers
    prevB = torch.zeros(R, ds)
    xcs, convs, yzs = [], [], []
    for t in range(S):
        sh = 1 if mutant == "taps_shifted" else 0
        if t < S0:
            taps = [inp(t - 3 + k - sh, taps=True) for k in range(4)]
            off = 1 if mutant == "conv_state_off_by_one" and t == S0 - 1 else 0
            new = torch.stack([inp(t - 3 + k - off) for k in range(4)], dim=-1)
            if t == S0 - 1:
                conv_buf[S0 & 1] = new
        else:
            par = t & 1
            rd, wr = (par ^ 1 if mutant == "parity_wrong" else par), par ^ 1
            st = conv_buf[rd]
            new = torch.stack([st[..., 1], st[..., 2], st[..., 3], xBC[:, t]], dim=-1)
            taps = [st[..., k] for k in range(4)] if sh else [st[..., 1], st[..., 2], st[..., 3], xBC[:, t]]
        acc = b.expand(R, cd)
        for k in range(4):
            acc = acc + w[:, k] * taps[k]
        xc = _rb(acc / (1.0 + torch.exp(-acc)))
        x, B, C = xc[:, :di].reshape(R, nh, hp), xc[:, di:di + ds], xc[:, di + ds:]
        if mutant == "bc_exchanged":
            B, C = C, B
        if mutant == "b_prev":
            B, prevB = prevB, B
        v = dtc[:, t] + dtb
        thr = 2.0 if mutant == "softplus_wrong_threshold" else 20.0
        dt = torch.where(v <= thr, torch.log1p(torch.exp(torch.clamp(v, max=thr))), v)
        if mutant == "threshold_branch_clamped":
            dt = torch.clamp(dt, max=20.0)
        dA = torch.exp(dt * A)
        if t < S0:
            hs = torch.zeros_like(h) if mutant == "chunk_reset" and t > 0 and t % CHUNK == 0 else h
        else:
            hs = torch.zeros_like(h) if mutant == "no_carry" and t == S0 else ssm_buf[rd]
        hn = hs * dA[:, :, None, None] + ((B[:, None, :] * dt[:, :, None])[:, :, None, :] * x[..., None])
        if mutant == "drop_element" and t == arg[4]:
            hn[arg[0], arg[1], arg[2], arg[3]] = hs[arg[0], arg[1], arg[2], arg[3]]
        y = (hn * C[:, None, None, :]).sum(-1)
        if mutant != "no_d":
            y = y + x * Dv[None, :, None]
        if mutant != "y_not_rounded":
            y = _rb(y)
        zz = z[:, t].reshape(R, nh, hp)
        yzs.append((y * (zz * (1.0 / (1.0 + torch.exp(-zz))))).reshape(R, di))
        if t < S0:
            h = hn
            if t == S0 - 1:
                ssm_buf[S0 & 1] = _rb(h)
        else:
            conv_buf[wr] = new
            ssm_buf[wr] = _rb(hn)
        xcs.append(xc)
        convs.append(new)
    yz = torch.stack(yzs, dim=1)
    rstd = 1.0 / torch.sqrt((yz * yz).mean(-1, keepdim=True) + NORM_EPS)
    out = _rb((yz * rstd) * nw)
    return dict(xc=torch.stack(xcs, 1).double().numpy(), conv=torch.stack(convs, 1).double().numpy(),
                ssm=ssm_buf[S & 1].double().numpy(), yz=yz.double().numpy(), out=out.double().numpy())


# ---------------------------------------------------------------------------- cases
def hot_indices(hp, ds):
    """d_state indices on the edges of the kernels' per-thread element ranges."""
    ept = ds // (THREADS // hp)
    s = {0, 7, 8, 15, 16, ept - 1, ept, 2 * ept - 1, ds // 2 - 1, ds // 2, ds - ept - 1, ds - ept, ds - 9, ds - 8,
         ds - 1}
    return sorted(i for i in s if 0 <= i < ds)


def impulse_times(S):
    return sorted({t for t in (0, 1, 2, 3, 15, 16, 17, S - 4, S - 3, S - 2, S - 1) if 0 <= t < S})


@dataclass
class Case:
    name: str
    hp: int
    ds: int
    S: int
    zx: np.ndarray                # fp64 [R][S][ncol], bf16 values on a 2^-10 grid
    P: Params
    probe_row: int
    b_hot: list                   # per step: the hot d_state index of B / of C on the probe row
    c_hot: list
    impulses: list                # (t, row, x channel)
    _refs: dict = field(default_factory=dict)

    @property
    def di(self):
        return NH * self.hp

    @property
    def conv_dim(self):
        return self.di + 2 * self.ds

    @property
    def ncol(self):
        return 2 * self.di + 2 * self.ds + NH

    def ref(self, S0, f32_term=F32_TERM, sharp=True) -> Ref:
        """The reference of prefill(S0) + steps, computed once and shared."""
        key = (S0, f32_term, sharp)
        if key not in self._refs:
            self._refs[key] = reference(self.zx, self.P, round_at=round_points(self.S, S0), f32_term=f32_term,
                                        sharp=sharp)
        return self._refs[key]


def _grid(a):
    """bf16 values on the 2^-10 grid; no -0.0 (a slab sum gives +0.0, and conv states are compared bit for bit)."""
    return bf(np.round(np.asarray(a, dtype=np.float64) * 1024.0) / 1024.0) + 0.0


def make_case(hp, ds, S) -> Case:
    rng = np.random.default_rng([hp, ds, S])
    R, nh = ROWS, NH
    di, cd = nh * hp, nh * hp + 2 * ds
    ncol = 2 * di + 2 * ds + nh
    w = rng.uniform(-0.6, 0.6, size=(cd, 4))
    while True:                    # neither symmetric nor shift-invariant (check_properties)
        bad = (np.abs(w - w[:, ::-1]).max(1) <= 0.1) | (np.abs(w[:, 1:] - w[:, :-1]).max(1) <= 0.1)
        if not bad.any():
            break
        w[bad] = rng.uniform(-0.6, 0.6, size=(int(bad.sum()), 4))
    w[di:] = np.array([0.03, -0.05, 0.07, 1.0]) + rng.uniform(-1, 1, size=(2 * ds, 4)) * np.array([.02, .02, .02, .1])
    P = Params(conv_w=w.astype(np.float32), conv_b=rng.uniform(-0.1, 0.1, size=cd).astype(np.float32),
               A=np.array([-2.0 ** -9, -16.0, -0.4, -1.0], dtype=np.float32),
               dt_bias=np.array([0.0, 1.0, 20.0, -1.5], dtype=np.float32),
               D=np.array([0.0, -2.5, 0.0, 1.75], dtype=np.float32),
               norm_w=rng.uniform(0.5, 1.5, size=di).astype(np.float32))
    zx = np.zeros((R, S, ncol))
    zx[..., :di] = 1.5 * rng.standard_normal((R, S, di))                             # z
    zx[..., di:2 * di] = rng.uniform(-1, 1, size=(R, S, di))                         # x
    zx[..., 2 * di:2 * di + 2 * ds] = rng.standard_normal((R, S, 2 * ds))            # B, C
    dt = rng.uniform(-2, 2, size=(R, S, nh))
    sign = np.where((np.arange(R)[:, None] + np.arange(S)[None, :]) % 2 == 0, 1.0, -1.0)
    dt[..., 1] = rng.uniform(1.5, 3.5, size=(R, S))
    dt[..., 2] = sign * rng.uniform(3, 4, size=(R, S))
    zx[..., 2 * di + 2 * ds:] = dt
    imp = [(t, r, (5 * t + 3 * r + 1) % di) for t in impulse_times(S) for r in range(R)]
    for t, r, ch in imp:
        zx[r, t, di + ch] = 6.0
    H = hot_indices(hp, ds)
    b_hot = [H[t % len(H)] for t in range(S)]
    c_hot = [b_hot[t - t % 3] for t in range(S)]
    pr = R - 1
    zx[pr, :, 2 * di:2 * di + 2 * ds] = -24.0
    for t in range(S):
        zx[pr, t, 2 * di + b_hot[t]] = 6.0
        zx[pr, t, 2 * di + ds + c_hot[t]] = 6.0
    return Case(f"hp{hp}-ds{ds}-S{S}", hp, ds, S, _grid(zx), P, pr, b_hot, c_hot, imp)


_CASES = {}


def cases():
    """{(hp, ds, S): Case} over GEOMS x LENGTHS, built once."""
    if not _CASES:
        for hp, ds in GEOMS:
            for S in LENGTHS:
                _CASES[hp, ds, S] = make_case(hp, ds, S)
    return _CASES


def slabs(zx, gs, seed=0):
    """fp32 [gs][...] whose sum in the kernels' order (v0 + v1 + ...) is zx exactly, every partial sum included:
    all values are multiples of 2^-10 below 2^7."""
    rng = np.random.default_rng([seed, gs])
    parts = [rng.integers(-4096, 4097, size=zx.shape) / 1024.0 for _ in range(gs - 1)]
    parts.append(zx - sum(parts))
    out = np.stack(parts).astype(np.float32)
    assert np.array_equal(out.astype(np.float64), np.stack(parts))
    acc = out[0].copy()
    for p in out[1:]:
        acc = acc + p
    assert acc.dtype == np.float32 and np.array_equal(acc.astype(np.float64), zx)
    return out


def drop_target(case: Case):
    """(row, head, p, n, t) of the state element whose update the drop_element mutant leaves out, and the step
    and yz channel that name it: the probe row's slow head, the hot element B writes at t (t % 3 == 0, so C
    reads it at t, t + 1 and t + 2), the head row p with the largest |x| at t."""
    t = 3 * (((case.S - 1) // 3) // 2)
    x = case.ref(case.S).xc[case.probe_row, t, :case.hp]
    p = int(np.argmax(np.abs(x)))
    return (case.probe_row, 0, p, case.b_hot[t], t), (case.probe_row, t, p)


def check_properties(case: Case):
    """What the module docstring claims of a case."""
    P, S, di, ds, hp = case.P, case.S, case.di, case.ds, case.hp
    ref = case.ref(S)
    dt = _softplus_thr(case.zx[..., 2 * di + 2 * ds:] + P.dt_bias.astype(np.float64))
    dA = np.exp(dt * P.A.astype(np.float64))
    assert dA[..., 0].min() >= 1 - 1e-2, "slow head"
    assert dA[..., 1].max() <= 0.02 and dA[..., 2].max() <= 0.02, "fast heads forget within a step"
    v = case.zx[..., 2 * di + 2 * ds + 2] + float(P.dt_bias[2])
    assert (v > 20.5).any() and (v < 19.5).any(), "head 2 on both sides of the softplus threshold"
    for a in (P.A, P.dt_bias):
        assert len(set(a.tolist())) == NH
    assert (P.D == 0).sum() == 2 and (P.D > 1).any() and (P.D < -1).any()
    w = P.conv_w.astype(np.float64)
    assert len({tuple(r) for r in w.tolist()}) == w.shape[0], "taps distinct per channel"
    assert (np.abs(w - w[:, ::-1]).max(1) > 0.05).all(), "taps not symmetric"
    assert (np.abs(w[:, 1:] - w[:, :-1]).max(1) > 0.02).all(), "a shifted tap is another tap"
    B, C = ref.xc[case.probe_row, :, di:di + ds], ref.xc[case.probe_row, :, di + ds:]
    for t in range(S):
        for a, hot in ((B, case.b_hot[t]), (C, case.c_hot[t])):
            assert a[t, hot] > 1.0 and np.abs(np.delete(a[t], hot)).max() < 1e-5 * a[t, hot], (case.name, t)
    if S >= 33:
        assert set(case.b_hot) == set(hot_indices(hp, ds)) == set(case.c_hot) | set(case.b_hot)
        assert any(case.c_hot[t] != case.b_hot[t] for t in range(S)), "C reads back an earlier B"
    assert {t for t, _, _ in case.impulses} == set(impulse_times(S))
    for t, r, ch in case.impulses:
        assert case.zx[r, t, di + ch] == 6.0
    rows = case.zx.reshape(ROWS, -1)                  # index separation: rows, heads (z included) all differ
    assert all(not np.array_equal(rows[i], rows[j]) for i in range(ROWS) for j in range(i))
    for blk in (case.zx[..., :di], case.zx[..., di:2 * di]):
        hd = blk.reshape(ROWS, S, NH, hp)
        assert all(not np.array_equal(hd[:, :, i], hd[:, :, j]) for i in range(NH) for j in range(i))
