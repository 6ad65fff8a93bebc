"""GEMM / GEMV test inputs on which every product is an integer, an exact reference, guarded buffers, the case
table of tests/test_gpu_gemm_probe.py and an fp32 restatement with mutant switches (CPU; numpy / torch only;
zonos_amd/csrc/gemm.hip and gemm_pf.hip are what they describe).

**Exact inputs.** A and W hold bf16 values on an integer grid, nonzero everywhere, a different draw per row and
column: {+-1, +-2, +-3} for the fp32 outputs (kind "i3"), {+-1} for the bf16 epilogues ("pm1"; the gate rows of
a SwiGLU weight are scaled by 2^-4, a power of two, so every pre-activation is still an exact multiple of one
quantum). Every product is an integer (times the quantum) and every partial sum at K <= 8192 stays far below
2^24, so fp32 accumulation is exact in any order, in any split, through MFMA or not. The reference is an integer
matrix product (evaluated in fp32 / fp64 BLAS, where the same argument makes it exact; check_properties()
asserts the magnitude).

**Criterion** (compare()). fp32 outputs -- every split-K slab of zk_gemm_bf16 mode 0, the mode 0 output of
zk_gemv_fused -- are bit-equal to the reference. There is no tolerance: a dropped, duplicated or misplaced
product of any size changes an integer. The bf16 epilogues follow from the kernels' rounding points in fp64
(bf / ulp / round_err of tests/mamba_probe.py):
  residual (zk_gemv_fused mode 2)  bf(res + bf(proj)): bit-equal (res is an integer, so the fp32 sum is exact);
  SwiGLU (mode 1)                  bf(bf(y) * bf(silu(bf(g)))): bit-equal, except where the fp32
      g / (1 + expf(-g)) can land on the other side of a bf16 midpoint (round_err with the fp32 term
      mamba_probe.F32_TERM: the same expression, measured there). There, and nowhere else, silu may be the
      neighbouring bf16 value: the output is then bf(bf(y) * that value), nothing else.
**Sensitivity** (check_properties()). A unit change of a pre-activation must stay visible after the bf16
roundings: the share of output elements whose expected value is unchanged by a move of one quantum (either
pre-activation, either direction) is <= 1 %, and the share of elements at which a flip is permitted <= 1e-3.
Plain +-1 draws do not meet that (measured on the CPU: 5 - 15 % of the SwiGLU outputs insensitive), for three
reasons, each met by the construction (layout(), make_data()):
  * a sum of an even number of +-1 is even, and y = 0 or gate = 0 (2 - 5 % of the elements each) gives 0 whatever
    the other is: one column of A holds +-2, so every sum is odd and never 0 (with the prologue: an odd number of
    odd activations among the free positions);
  * silu has its minimum at g = -1.28, where one quantum of the gate moves it by less than a bf16 spacing, and
    g = 95 / 16 is the one gate value in +-25 at which a flip is permitted: two columns with A = +1 in every row
    and a gate weight of +24 quanta each (W_y opposite in the two, so y gets nothing) put the gate at 3 +
    noise, and all but FREE_GATE of the other positions cancel in pairs (below) in the gate columns, so the gate
    stays within 3 +- 3 (FREE_GATE_LN with the prologue, whose activations reach +-3);
  * at K > 2048 a +-1 sum reaches the magnitudes (|y| >= 128, |proj| >= 256) at which one quantum is less than
    the spacing of the bf16 result: all but FREE_K (prologue: FREE_K_LN) of the k positions are paired by a
    fixed random involution pi with A[m][pi k] = q_k A[m][k] and W[n][pi k] = -q_k W[n][k], so the two products
    cancel in every (m, n), the sums are those of the free positions at every K, and each single product still
    counts one quantum. The pairing is random over k, so no k-step, chunk or K range of a wave holds only whole
    pairs, and a product computed with the wrong partner (a stale chunk, a neighbouring row) does not cancel.
With it the largest insensitive share of a case is 5.4e-4 and the largest permitted-flip share 1.3e-4.

**LayerNorm prologue** (zk_gemv_fused with ln_w, K = 2048). Row m holds c_m + s_m on a random half of the
positions and c_m - s_m on the others ((c, s) different per row), so (x - mean) * rstd is +-1 to within 1e-5;
ln_w in {+-1, +-2}, ln_b in {0, +-1, +-2} with |ln_b| != |ln_w|, so the bf16 activation is the exactly known
nonzero integer +-ln_w + ln_b: the GEMV behind the prologue is bit-exact and a ln_w / ln_b read from a
neighbouring k shows. A wrong mean or variance does not (the tolerance tests of tests/test_gpu_ops.py see it).

**Buffers** (make_a(), make_out(), check_guards()). A is allocated [M + 2][lda] with NaN in the rows >= M and in
the columns K .. lda - 1 of every row (view "last3": [M + 2][3][K], A pointing at the last K of each row, the first
two NaN -- the heads GEMM's view of the last prefill row, lda = 3 K). Outputs carry a guard band of a fixed
non-NaN bit pattern before and after and are prefilled inside with a NaN of a payload no arithmetic produces
(the residual output holds the residual instead). check_guards() verifies that no guard word changed and that
every inside element was written.

**emulate()** restates a tiled split-K GEMM over the packed weight image (pack_weights():
[Npad/16][K/32][64 lanes][8], rows padded to 64) in fp32 torch, writing the same buffers. `mutant=` switches one
deliberate error on (MUTANTS; mutant_applies() names the cases each is aimed at);
tests/test_gemm_probe_cpu.py shows that each fails the criterion or the guards on every such case.

**Cases** (CASES). Each names the instantiation it is there for (`want`: fields of zk_gemm_plan /
zk_gemv_plan); the CPU test checks every claim against the library and that the union covers the selector
tuples listed in REQUIRED.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np
import torch

from tests.mamba_probe import F32_TERM, bf, round_err, ulp

GATE_Q = 2.0 ** -4                      # quantum of the SwiGLU gate pre-activation
FREE_K, FREE_K_LN = 2048, 512           # free (unpaired) k positions of a bf16-epilogue case (LayerNorm: |a| <= 3)
FREE_GATE, FREE_GATE_LN, GATE_OFFSET = 128, 32, 48   # ... of a SwiGLU's gate columns; the gate's offset in quanta
GUARD_F32, GUARD_BF16 = 0x5A5A5A5A, 0x5A5A          # guard words (1.5e16, 1.5e16)
UNSET_F32, UNSET_BF16 = 0x7FC0BEEF, 0x7FD5          # prefill inside the outputs: NaNs with a payload
POISON_BF16 = 0x7FC1                                # around A
MAX_SHARE_INSENSITIVE, MAX_SHARE_FLIP = 1e-2, 1e-3

MUTANTS = ("drop_last_kstep", "stale_chunk", "lda_ignored", "row_clamp_stored", "col_tail_overrun",
           "tile_past_n_stored", "split_slab_stride", "y_gate_swapped", "swiglu_pair_shift",
           "residual_row_neighbour", "ln_w_neighbour", "skip_ignored", "skip_partial")


# ---------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    entry: str                      # "gemm" (zk_gemm_bf16) or "gemv" (zk_gemv_fused)
    M: int
    N: int
    K: int
    nsplit: int = 1
    mode: int = 0
    ln: bool = False
    lda: int = 0                    # 0: K
    view: str = "dense"             # "last3": lda = 3 K, A at the last K of each [3][K] row
    skip: bool = False              # the skip-word case: a launch with the word 1, then one with 0
    want: tuple = ()                # ((plan field, value), ...) the case is there for

    @property
    def row_stride(self):
        return 3 * self.K if self.view == "last3" else (self.lda or self.K)

    @property
    def a_off(self):
        return 2 * self.K if self.view == "last3" else 0

    @property
    def kind(self):
        return "i3" if self.mode == 0 else "pm1"

    @property
    def free_k(self):
        """k positions whose products do not cancel in pairs (module docstring)."""
        return self.K if self.mode == 0 else min(self.K, FREE_K_LN if self.ln else FREE_K)

    @property
    def paired(self):
        return self.free_k < self.K

    @property
    def ncol(self):
        return self.N // 2 if self.mode == 1 else self.N

    @property
    def name(self):
        s = f"{self.entry}{self.mode}-M{self.M}-N{self.N}-K{self.K}"
        s += f"-s{self.nsplit}" if self.nsplit > 1 else ""
        s += "-ln" if self.ln else ""
        s += f"-lda{self.row_stride}" if self.row_stride != self.K else ""
        return s + ("-skip" if self.skip else "")


def _w(**kw):
    return tuple(sorted(kw.items()))


def _cases():
    c = []
    g = lambda *a, **k: c.append(Case("gemm", *a, **k))          # noqa: E731
    # ---- zk_gemm_bf16 mode 0, k_gemv_rk: ks x M, N % 32 in {0, 8, 17} in turn (the second tile of a
    # workgroup wholly or partly past N)
    for i, ks in enumerate((1, 2, 4, 8, 16)):
        for j, M in enumerate((1, 15, 16)):
            ns = 1 + (i + j) % 2
            g(M, (96, 104, 113)[(i + j) % 3], ks * 128 * ns, ns, want=_w(family="rk", ks=ks))
    # ---- k_gemm_ws: chunks at mt = 8
    for i, nch in enumerate((2, 4, 8, 16, 32)):
        ns = (1, 2)[i % 2]
        g(128 - i % 2, 200, nch * 64 * ns, ns, want=_w(family="ws", nchunks=nch, mt=8))
    # row edges of the 16-row tile counts
    for M, mt in ((17, 2), (32, 2), (33, 4), (64, 4), (65, 8), (127, 8), (128, 8)):
        g(M, 136, 128 * (1 + M % 2), 1 + M % 2, want=_w(family="ws", nchunks=2, mt=mt))
    # compute waves per workgroup (ws_ncw at nsplit = 8), N in three forms: N % 4 == 0 with a partial last
    # workgroup, N % 4 != 0 (register stores; the scalar tail), a 16-column tile wholly past N
    for ncw, Ns in ((2, (1000, 1001, 1003)), (3, (1100, 1080, 1101, 1102)), (4, (1552, 1553, 1555)),
                    (5, (2072, 2056, 2073, 2075))):
        for N in Ns:
            g(128, N, 1024, 8, want=_w(family="ws", nchunks=2, mt=8, ncw=ncw))
    # (The scalar tail of the LDS-staged store path cannot be reached: that path runs only at N % 4 == 0, where
    # a lane's first column n0 + c4 and N are both multiples of 4, so fewer than 4 columns never remain.)
    # ---- k_gemm: ring slots x tiles per wave, a second row block of one row, N no multiple of 64 ntw
    for u, nch in ((1, 3), (2, 6), (4, 4)):
        g(129, 200, nch * 64, 1, want=_w(family="tile", u=u, ntw=1, nchunks=nch))
        g(129, 600, nch * 64 * 2, 2, want=_w(family="tile", u=u, ntw=2, nchunks=nch))
    g(40, 200, 192, 1, want=_w(family="tile", u=1, ntw=1, nchunks=3))       # decode regime, falls through
    # ---- k_gemm_pf: 256 tiles, a last row block of one row
    g(15 * 256 + 1, 4096, 128, 1, want=_w(family="pf", pf_cols=256, gx=256))
    # ---- mode 1 (SwiGLU)
    for ks, M in ((4, 1), (8, 15), (16, 16)):
        g(M, 112, ks * 128, 1, 1, want=_w(family="rk", ks=ks))
    g(16, 112, 256, 1, 1, want=_w(family="ws", nchunks=4, mt=1))
    for i, (M, mt) in enumerate(((17, 2), (33, 4), (100, 8))):
        for nch in (4, 8, 16, 32):
            g(M + (nch == 32), 208, nch * 64, 1, 1, want=_w(family="ws", nchunks=nch, mt=mt))
    for u, nch in ((1, 3), (2, 6), (4, 4)):
        g(129, 208, nch * 64, 1, 1, want=_w(family="tile", u=u, ntw=1))
    g(15 * 256 + 1, 4096, 128, 1, 1, want=_w(family="pf", pf_cols=256, gx=256))
    g(7 * 256 + 1, 8256, 128, 1, 1, want=_w(family="pf", pf_cols=256, gx=264))   # partial last column tile
    # ---- zk_gemv_fused: every (mode, LayerNorm, layout, K, rows) the library instantiates, N at the layout
    # edges (255 / 256 tiles, 511 / 512 tiles, an odd tile count of the two-tile layout, N % 16 != 0 for mode 0)
    v = lambda *a, **k: c.append(Case("gemv", *a, **k))          # noqa: E731
    i = 0
    for K in (2048, 4096, 8192):
        for ln in ((False, True) if K == 2048 else (False,)):
            for mode in (0, 1, 2):
                for lay in (0, 1, 2):
                    if lay == 0 and (mode == 1 or ln):
                        continue
                    if lay == 0:
                        Ns = (4080, 203 if mode == 0 else 200)
                    elif lay == 1:
                        Ns = (8176, 208 if (mode == 1 or ln) else 4096)
                    else:
                        Ns = (8192, 8208)
                    # both row counts of each image (M = 1: every clamped row is row 0, and with the prologue
                    # one wave alone loads a row; M = 16: no clamp), the two N of the layout in turn
                    i += 1
                    for xi, (xr, Ms) in enumerate(((2, (1, 2)), (16, (3, 16)))):
                        for j, M in enumerate(Ms):
                            v(M, Ns[(i + xi + j) % 2], K, 1, mode, ln, want=_w(lay=lay, ksw=K // 32, xr=xr))
    v(5, 8200, 2048, want=_w(lay=2, ksw=64, xr=16))                # two-tile layout, N % 16 != 0
    # ---- lda: every family with lda = K + 8, and the heads GEMM's view of the last prefill row
    g(15, 104, 256, 1, lda=264, want=_w(family="rk", ks=2))
    g(65, 1001, 256, 2, lda=264, want=_w(family="ws", nchunks=2, mt=8))
    g(129, 200, 192, 1, lda=200, want=_w(family="tile", u=1))
    g(15 * 256 + 1, 4096, 128, 1, lda=136, want=_w(family="pf"))
    g(33, 208, 256, 1, 1, lda=264, want=_w(family="ws", nchunks=4, mt=4))
    v(3, 203, 2048, lda=2056, want=_w(lay=0))
    v(2, 208, 2048, 1, 0, True, lda=2056, want=_w(lay=1))
    v(2, 200, 4096, 1, 2, lda=4104, want=_w(lay=0, xr=2))
    g(8, 1003, 256, 2, view="last3", want=_w(family="rk", ks=1))
    g(20, 1003, 256, 2, view="last3", want=_w(family="ws", nchunks=2, mt=2))
    v(2, 203, 2048, view="last3", want=_w(lay=0))
    # ---- the skip word: every family with the word 1, then 0
    g(15, 113, 256, 1, skip=True, want=_w(family="rk"))
    g(65, 1001, 256, 2, skip=True, want=_w(family="ws"))
    g(129, 200, 192, 1, skip=True, want=_w(family="tile"))
    g(15 * 256 + 1, 4096, 128, 1, skip=True, want=_w(family="pf"))
    g(33, 208, 256, 1, 1, skip=True, want=_w(family="ws"))
    v(3, 203, 2048, skip=True, want=_w(lay=0))
    v(2, 208, 2048, 1, 1, True, skip=True, want=_w(lay=1))
    v(16, 200, 2048, 1, 2, skip=True, want=_w(lay=0))
    return tuple(c)


CASES = _cases()

# The selector tuples the cases together must run: (entry, mode, ((field, value), ...)).
REQUIRED = (
    [("gemm", 0, _w(family="rk", ks=ks)) for ks in (1, 2, 4, 8, 16)]
    + [("gemm", 0, _w(family="ws", nchunks=n, mt=8)) for n in (2, 4, 8, 16, 32)]
    + [("gemm", 0, _w(family="ws", mt=mt)) for mt in (2, 4, 8)]
    + [("gemm", 0, _w(family="ws", ncw=n)) for n in (2, 3, 4, 5)]
    + [("gemm", 0, _w(family="ws", gz=z)) for z in (1, 2, 8)]
    + [("gemm", 0, _w(family="tile", u=u, ntw=t)) for u in (1, 2, 4) for t in (1, 2)]
    + [("gemm", 0, _w(family="pf", pf_cols=256))]
    + [("gemm", 1, _w(family="rk", ks=ks)) for ks in (4, 8, 16)]
    + [("gemm", 1, _w(family="ws", nchunks=4, mt=1))]
    + [("gemm", 1, _w(family="ws", nchunks=n, mt=mt)) for n in (4, 8, 16, 32) for mt in (2, 4, 8)]
    + [("gemm", 1, _w(family="tile", u=u)) for u in (1, 2, 4)]
    + [("gemm", 1, _w(family="pf", pf_cols=256))]
    + [("gemv", m, _w(lay=lay, ksw=ksw, xr=xr)) for m in (0, 1, 2) for lay in (0, 1, 2) for ksw in (64, 128, 256)
       for xr in (2, 16) if not (lay == 0 and m == 1)]
)
REQUIRED_LN = [(m, _w(lay=lay, ksw=64, xr=xr)) for m in (0, 1, 2) for lay in (1, 2) for xr in (2, 16)]


# ---------------------------------------------------------------------------- data
def _signed(rng, shape, hi):
    """int8 values in {+-1 .. +-hi}, uniform."""
    v = rng.integers(1, hi + 1, size=shape, dtype=np.int8)
    return np.where(rng.integers(0, 2, size=shape, dtype=np.int8) == 1, v, -v).astype(np.int8)


@dataclass(frozen=True)
class Layout:
    """The k positions of a bf16-epilogue case (module docstring, "Sensitivity")."""
    free: np.ndarray        # free for every column (FREE_GATE of them for a SwiGLU, else the case's free_k)
    ea: np.ndarray          # pairs (ea, eb): they cancel in the gate columns only (free for y)
    eb: np.ndarray
    pa: np.ndarray          # pairs (pa, pb): they cancel in every column
    pb: np.ndarray
    q: np.ndarray           # q of the pairs (ea | pa): A[pi k] = q A[k]; with the LayerNorm prologue -1 throughout
    k1: int                 # SwiGLU without the prologue: the column of +-2 in A (every sum odd)
    k2: int                 # SwiGLU: A[k2] = A[k3] = +1 in every row, W_gate = +GATE_OFFSET / 2 each,
    k3: int                 # W_y[k3] = -W_y[k2]: the gate's offset, nothing in y


@functools.lru_cache(maxsize=16)
def layout(K, free_y, mode, ln) -> Layout:
    rng = np.random.default_rng(7000 + K + 3 * free_y + mode)
    perm = rng.permutation(K)
    fg = min(FREE_GATE_LN if ln else FREE_GATE, free_y) if mode == 1 else free_y
    free, e, p = perm[:fg], perm[fg:free_y], perm[free_y:]
    he, hp = len(e) // 2, len(p) // 2
    q = -np.ones(he + hp, dtype=np.int8) if ln else _signed(rng, he + hp, 1)
    return Layout(np.sort(free[3:]) if mode == 1 else np.sort(free), e[:he], e[he:], p[:hp], p[hp:], q,
                  int(free[0]), int(free[1]), int(free[2]))


def _gate_rows(n):
    return (np.arange(n) % 16) >= 8


@functools.lru_cache(maxsize=6)
def _bank(kind, K, rows, free_y, mode, ln):
    """The weight draws: int8 [rows][K]; the gate rows of a SwiGLU weight in quanta of GATE_Q. Cases of one
    (kind, K) with many rows share the first N of these."""
    rng = np.random.default_rng({"i3": 11, "pm1": 13}[kind] * 100003 + K)
    w = _signed(rng, (rows, K), 3 if kind == "i3" else 1)
    if mode == 0:
        return w
    L = layout(K, free_y, mode, ln)
    nq = len(L.ea)
    w[:, L.pb] = -w[:, L.pa] * L.q[nq:]
    if mode == 1:
        g = _gate_rows(rows)
        w[np.ix_(g, L.eb)] = -w[np.ix_(g, L.ea)] * L.q[:nq]
        w[:, L.k3] = -w[:, L.k2]
        _set_offset(w, L)
    return w


def _set_offset(w, L):
    g = _gate_rows(len(w))
    w[g, L.k2] = w[g, L.k3] = GATE_OFFSET // 2


@dataclass
class Data:
    A: np.ndarray                   # int8 [M][K] -- with ln: the input rows x of the prologue (c +- s)
    W: np.ndarray                   # int8 [N][K]; mode 1: rows in the kernels' interleaved order, each group of
                                    # 16 = y[f0 .. f0+7], gate[f0 .. f0+7]; the gate rows count GATE_Q each
    res: np.ndarray | None = None   # mode 2: int8 [M][N]
    ln_w: np.ndarray | None = None  # int8 [K]
    ln_b: np.ndarray | None = None
    act: np.ndarray | None = None   # with ln: the bf16 activation the prologue must produce, int8 [M][K]
    extra: dict = field(default_factory=dict)


def make_data(case: Case, which: int) -> Data:
    """Data set `which` (0, 1) of a case: A drawn anew, W the bank's rows -- for which = 1 rotated by 16 rows and
    negated, so no column, row or sign of the first set is right for the second."""
    rng = np.random.default_rng(1000 * which + 17 * case.M + case.N + case.K + 3 * case.mode)
    M, K = case.M, case.K
    rows = case.N if case.N <= 2112 else 8256
    W = _bank(case.kind, K, rows, case.free_k, case.mode, case.ln)[:case.N]
    L = layout(K, case.free_k, case.mode, case.ln) if case.mode else None
    if which:
        W = -np.roll(W, 16, axis=0)
        if case.mode == 1:
            _set_offset(W, L)
    d = Data(A=None, W=W)
    if case.mode:
        pair_a, pair_b = np.concatenate([L.ea, L.pa]), np.concatenate([L.eb, L.pb])
    if case.ln:
        cs = [(c, s) for s in (1, 2, 4, 8) for c in (-3, -2, -1, 0, 1, 2, 3)]
        pick = rng.permutation(len(cs))[:M]
        c = np.array([cs[p][0] for p in pick], dtype=np.int8)[:, None]
        s = np.array([cs[p][1] for p in pick], dtype=np.int8)[:, None]
        d.ln_w = _signed(rng, K, 2)
        mag = np.where(np.abs(d.ln_w) == 1, 2, 1).astype(np.int8)       # |ln_b| != |ln_w|, or 0
        d.ln_b = (mag * rng.integers(-1, 2, size=K, dtype=np.int8)).astype(np.int8)
        sign = np.ones((M, K), dtype=np.int8)
        if case.mode == 0:
            for m in range(M):
                sign[m, rng.permutation(K)[:K // 2]] = -1
        else:
            # a[pi k] = -a[k] in every row: the opposite sign, the same ln_w, the opposite ln_b. SwiGLU: the
            # offset columns hold a = -ln_w + ln_b = +1 in every row, and an odd number of odd activations
            # among the free positions makes every sum odd (neither y nor the gate is ever 0).
            free, fixed = L.free, 0
            if case.mode == 1:
                free, fixed = np.concatenate([L.free, [L.k1]]), 2
                d.ln_w[[L.k2, L.k3]], d.ln_b[[L.k2, L.k3]] = 1, 2
                sign[:, [L.k2, L.k3]] = -1
            d.ln_w[pair_b], d.ln_b[pair_b] = d.ln_w[pair_a], -d.ln_b[pair_a]
            if case.mode == 1 and int(((d.ln_w[free] + d.ln_b[free]) % 2).sum()) % 2 == 0:
                f0 = free[0]
                d.ln_w[f0], d.ln_b[f0] = (2, 0) if (d.ln_w[f0] + d.ln_b[f0]) % 2 else (1, 0)
            for m in range(M):
                sign[m, free[rng.permutation(len(free))[:(len(free) - fixed) // 2]]] = -1
                sign[m, pair_a] = _signed(rng, len(pair_a), 1)
                sign[m, pair_b] = -sign[m, pair_a]
        d.A = (c + s * sign).astype(np.int8)
        d.act = (sign * d.ln_w[None, :] + d.ln_b[None, :]).astype(np.int8)
        d.extra = dict(c=c, s=s, sign=sign)
    else:
        d.A = _signed(rng, (M, K), 3 if case.kind == "i3" else 1)
        if case.mode:
            d.A[:, pair_b] = d.A[:, pair_a] * L.q
        if case.mode == 1:
            d.A[:, L.k1] *= 2              # one column of +-2: every sum is odd, neither y nor the gate is ever 0
            d.A[:, [L.k2, L.k3]] = 1
    if case.mode == 2:
        d.res = rng.integers(-8, 9, size=(M, case.N), dtype=np.int8)
    return d


def activation(d: Data) -> np.ndarray:
    return d.act if d.act is not None else d.A


def weight_values(case: Case, d: Data) -> torch.Tensor:
    """The nn.Linear weight [N][K] the entry is given (before packing), bf16: the draws, the gate rows of a
    SwiGLU weight times GATE_Q."""
    W = torch.from_numpy(d.W.astype(np.float32))
    if case.mode == 1:
        W = W * torch.where((torch.arange(case.N) % 16) >= 8, GATE_Q, 1.0)[:, None]
    return W.to(torch.bfloat16)


def pack_weights(W: np.ndarray) -> np.ndarray:
    """zk_pack_weights on the CPU: [N][K] -> [Npad/16][K/32][64][8], rows >= N zero."""
    N, K = W.shape
    Np = (N + 63) // 64 * 64
    full = np.zeros((Np, K), dtype=W.dtype)
    full[:N] = W
    # lane = 16 * kq + nl holds W[16 nt + nl][32 kc + 8 kq + e]
    return np.ascontiguousarray(full.reshape(Np // 16, 16, K // 32, 4, 8).transpose(0, 2, 3, 1, 4)
                                ).reshape(Np // 16, K // 32, 64, 8)


def unpack_weights(P: np.ndarray) -> np.ndarray:
    nt, kc = P.shape[:2]
    return np.ascontiguousarray(P.reshape(nt, kc, 4, 16, 8).transpose(0, 3, 1, 2, 4)).reshape(nt * 16, kc * 32)


# ---------------------------------------------------------------------------- reference and criterion
def _matmul_exact(A, W):
    """A . W^T of integer matrices as int64 (fp32 BLAS, exact: every partial sum is an integer < 2^24)."""
    out = (torch.from_numpy(A.astype(np.float32)) @ torch.from_numpy(W.astype(np.float32)).t()).numpy()
    assert np.abs(out).max() < 2 ** 23
    return out.astype(np.int64)


def _silu_points(g):
    """(bf(silu(bf g)), whether the fp32 evaluation may round the other way) in fp64."""
    bg = bf(g)
    s = bg / (1.0 + np.exp(-bg))
    sl, e = round_err(s, F32_TERM * 2.0 ** -24 * np.abs(s))
    return sl, e > 0


def _swiglu(y, g):
    sl, flip = _silu_points(g)
    return bf(bf(y) * sl), flip


def _split_yg(pre):
    """Interleaved columns [M][N] (int64 quanta) -> (y, g) [M][N/2] in their units."""
    M, N = pre.shape
    q = pre.reshape(M, N // 16, 2, 8)
    return q[:, :, 0].reshape(M, N // 2).astype(np.float64), q[:, :, 1].reshape(M, N // 2) * GATE_Q


@dataclass
class Expected:
    slabs: np.ndarray | None = None     # mode 0: int64 [nsplit][M][N]
    out: np.ndarray | None = None       # modes 1, 2: fp64 [M][ncol] (bf16 values)
    alt: tuple = ()                     # mode 1: the outputs with silu one bf16 step down / up
    flip: np.ndarray | None = None      # mode 1: where alt is admissible
    pre: np.ndarray | None = None       # int64 [M][N] pre-activations in quanta


def reference(case: Case, d: Data) -> Expected:
    A, W, ks = activation(d), d.W, case.K // case.nsplit
    if case.mode == 0:
        slabs = np.stack([_matmul_exact(A[:, s * ks:(s + 1) * ks], W[:, s * ks:(s + 1) * ks])
                          for s in range(case.nsplit)])
        return Expected(slabs=slabs, pre=slabs.sum(0))
    pre = _matmul_exact(A, W)
    if case.mode == 2:
        return Expected(out=bf(d.res.astype(np.float64) + bf(pre.astype(np.float64))), pre=pre)
    y, g = _split_yg(pre)
    sl, flip = _silu_points(g)
    by = bf(y)
    # silu's bf16 neighbours, by magnitude (below a power of two the spacing halves)
    mag, sg = np.abs(sl), np.sign(sl)
    dn, up = sg * (mag - ulp(mag * (1 - 2.0 ** -9))), sg * (mag + ulp(mag))
    return Expected(out=bf(by * sl), alt=(bf(by * dn), bf(by * up)), flip=flip, pre=pre)


def _bits(x, dtype):
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dtype)
    return t.view(torch.int32 if dtype == torch.float32 else torch.int16).numpy()


def compare(case: Case, exp: Expected, got: np.ndarray) -> dict:
    """The criterion. got: the inside of the output as integer bit patterns (int32 [nsplit][M][N] for the fp32
    outputs, int16 [M][ncol] for bf16). Raises AssertionError; returns the counts for the record."""
    if case.mode == 0:
        want = _bits(exp.slabs, torch.float32)
        bad = want != got.reshape(want.shape)
        assert not bad.any(), f"{case.name}: {int(bad.sum())} of {bad.size} fp32 elements differ, first at " \
                              f"{tuple(np.argwhere(bad)[0])}"
        return dict(exact=int(bad.size), flips=0, permitted=0)
    want = _bits(exp.out, torch.bfloat16)
    got = got.reshape(want.shape)
    bad = want != got
    flips = 0
    if case.mode == 1:
        ok_alt = exp.flip & ((got == _bits(exp.alt[0], torch.bfloat16)) | (got == _bits(exp.alt[1], torch.bfloat16)))
        flips = int((bad & ok_alt).sum())
        bad &= ~ok_alt
    assert not bad.any(), f"{case.name}: {int(bad.sum())} of {bad.size} bf16 elements differ, first at " \
                          f"{tuple(np.argwhere(bad)[0])}"
    return dict(exact=int(bad.size) - flips, flips=flips, permitted=int(exp.flip.sum()) if case.mode == 1 else 0)


def check_properties(case: Case, d: Data, exp: Expected) -> dict:
    """What the module docstring claims of a case's inputs, asserted on the reference alone."""
    A, W = activation(d), d.W
    assert (A != 0).all() and (W != 0).all()
    assert np.abs(A).max() <= 3
    if case.kind == "i3":
        assert np.abs(W).max() <= 3
    else:
        # +-1 throughout, but for the SwiGLU's parity column of A and the gate's two offset columns of W
        assert (np.abs(W) != 1).sum() == (2 * _gate_rows(case.N).sum() if case.mode == 1 else 0)
        if not case.ln:
            assert (np.abs(A) != 1).sum() == (case.M if case.mode == 1 else 0)
    # a different draw per row and column: no two rows of A, no two of W, are parallel (strict Cauchy-Schwarz)
    for X in (A[:512], W[:512]):
        if len(X) > 1:
            X = X[:, :256].astype(np.int64)
            G, n2 = X @ X.T, (X * X).sum(1)
            strict = G * G < n2[:, None] * n2[None, :]
            np.fill_diagonal(strict, True)
            assert strict.all()
    # exactness: sum |a w| bounds every partial sum in any order
    bound = int(np.abs(A).astype(np.int64).max() * np.abs(W).astype(np.int64).max()) * case.K
    assert bound < 2 ** 24 and np.abs(exp.pre).max() < 2 ** 24
    out = dict(max_sum=int(np.abs(exp.pre).max()), insensitive=0.0, flip=0.0)
    if case.ln:
        x = d.A.astype(np.float64)
        n = (x - x.mean(1, keepdims=True)) / np.sqrt(x.var(1, keepdims=True) + 1e-5)
        assert np.abs(np.abs(n) - 1).max() < 1e-5
        pre = n * d.ln_w + d.ln_b
        r, u = bf(pre), ulp(pre)
        assert (r == d.act).all() and (d.act != 0).all()
        off = np.abs(pre - r)
        assert np.minimum(0.5 * u - off, 0.25 * u + off).min() > 2.0 ** -10        # far above 1e-5
        assert len({(int(c), int(s)) for c, s in zip(d.extra["c"][:, 0], d.extra["s"][:, 0])}) == case.M
        assert (d.extra["sign"].sum(1) == 0).all() and (np.abs(d.ln_w) != np.abs(d.ln_b)).all()
        # different per k: a ln_w / ln_b taken from k + 1 changes the activation at a good share of the positions
        shifted = d.extra["sign"] * np.roll(d.ln_w, -1) + d.ln_b
        assert (shifted != d.act).mean() > 0.3
    if case.mode == 0:
        return out
    # (a large M: the shares over the first and the last 128 rows)
    rows = np.arange(case.M) if case.M <= 256 else np.r_[0:128, case.M - 128:case.M]
    pre, ref = exp.pre[rows], exp.out[rows]
    same = np.zeros(ref.shape, dtype=bool)
    if case.mode == 2:
        for dlt in (-1, 1):
            same |= bf(d.res[rows] + bf((pre + dlt).astype(np.float64))) == ref
    else:
        y, g = _split_yg(pre)
        for dy, dg in ((-1, 0), (1, 0), (0, -GATE_Q), (0, GATE_Q)):
            same |= _swiglu(y + dy, g + dg)[0] == ref
        out["flip"] = float(exp.flip.mean())
        assert out["flip"] <= MAX_SHARE_FLIP, (case.name, out["flip"])
    out["insensitive"] = float(same.mean())
    assert out["insensitive"] <= MAX_SHARE_INSENSITIVE, (case.name, out["insensitive"])
    return out


# ---------------------------------------------------------------------------- buffers
def _bf16_bits(x_int8):
    return torch.from_numpy(x_int8.astype(np.float32)).to(torch.bfloat16).view(torch.int16)


def make_a(case: Case, d: Data) -> torch.Tensor:
    """The A allocation as int16 bit patterns, flat [(M + 2) * row_stride]; the entry's A is element a_off."""
    rs = case.row_stride
    buf = torch.full((case.M + 2, rs), POISON_BF16, dtype=torch.int16)
    buf[:case.M, case.a_off:case.a_off + case.K] = _bf16_bits(d.A)
    return buf.reshape(-1)


def guard_len(case: Case) -> int:
    return max(4096, 2 * ((case.N + 63) // 64 * 64))


def inside_len(case: Case) -> int:
    return case.nsplit * case.M * case.ncol


def make_out(case: Case, d: Data) -> torch.Tensor:
    """The output allocation as bit patterns (int32 for fp32 outputs, int16 for bf16): guard | inside | guard."""
    f32 = case.mode == 0
    G, n = guard_len(case), inside_len(case)
    buf = torch.full((2 * G + n,), GUARD_F32 if f32 else GUARD_BF16, dtype=torch.int32 if f32 else torch.int16)
    buf[G:G + n] = _bf16_bits(d.res).reshape(-1) if case.mode == 2 else (UNSET_F32 if f32 else UNSET_BF16)
    return buf


def inside(case: Case, buf) -> np.ndarray:
    G = guard_len(case)
    return buf[G:G + inside_len(case)].cpu().numpy()


def check_guards(case: Case, buf) -> None:
    f32 = case.mode == 0
    b = buf.cpu().numpy()
    G, n = guard_len(case), inside_len(case)
    for name, part in (("before", b[:G]), ("after", b[G + n:])):
        bad = np.flatnonzero(part != (GUARD_F32 if f32 else GUARD_BF16))
        assert bad.size == 0, f"{case.name}: {bad.size} guard words {name} the output changed, first at {bad[0]}"
    if case.mode != 2:
        unset = np.flatnonzero(b[G:G + n] == (UNSET_F32 if f32 else np.int16(UNSET_BF16)))
        assert unset.size == 0, f"{case.name}: {unset.size} output elements never written, first at {unset[0]}"


# ---------------------------------------------------------------------------- the restatement
def mutant_applies(mutant: str, case: Case) -> bool:
    """Whether `mutant` is aimed at `case` (it must then fail the criterion or the guards)."""
    if case.skip:
        return mutant in ("skip_ignored", "skip_partial")
    return {
        "drop_last_kstep": True,
        "stale_chunk": case.K // case.nsplit >= 128,
        "lda_ignored": case.row_stride != case.K and case.M > 1,
        "row_clamp_stored": True,
        "col_tail_overrun": case.mode == 0 and case.N % 4 != 0,
        # (not the residual epilogue: the packed image is zero past N, so x += 0 there changes nothing)
        "tile_past_n_stored": case.mode == 0 and case.N % 16 != 0 or case.mode == 1 and case.N % 64 != 0,
        "split_slab_stride": case.nsplit > 1 and case.N % 64 != 0,
        "y_gate_swapped": case.mode == 1,
        "swiglu_pair_shift": case.mode == 1 and case.N > 16,
        "residual_row_neighbour": case.mode == 2 and case.M > 1,
        "ln_w_neighbour": case.ln,
        "skip_ignored": False,
        "skip_partial": False,
    }[mutant]


def _f32_bits(t):
    return t.contiguous().view(torch.int32)


def emulate(case: Case, d: Data, a_buf: torch.Tensor, packed: np.ndarray, out: torch.Tensor, skip_word: int = 0,
            mutant: str | None = None) -> None:
    """A tiled split-K GEMM in fp32 torch over the buffers of make_a() / pack_weights() / make_out(): column
    tiles of 16, chunks of 64 (two k-steps of 32), rows in blocks of 16 clamped to row M - 1, one fp32 slab per
    split, the epilogues at the kernels' rounding points. Writes `out` in place."""
    assert mutant is None or mutant in MUTANTS
    M, N, K, ns = case.M, case.N, case.K, case.nsplit
    G = guard_len(case)
    if skip_word and mutant != "skip_ignored" and mutant != "skip_partial":
        return
    first_tile_only = bool(skip_word) and mutant == "skip_partial"
    Wu = torch.from_numpy(unpack_weights(packed).astype(np.float32))             # [Npad][K], rows >= N zero
    if case.mode == 1:
        Wu = Wu * torch.where((torch.arange(Wu.shape[0]) % 16) >= 8, GATE_Q, 1.0)[:, None]
    Np = Wu.shape[0]
    # ---- activation rows, through the row stride, rows >= M clamped (computed, not stored)
    Mp = (M // 16 + 1) * 16                                                      # (at least one row past M)
    rows = torch.clamp(torch.arange(Mp), max=M - 1)
    stride = K if mutant == "lda_ignored" else case.row_stride
    idx = case.a_off + rows[:, None] * stride + torch.arange(K)[None, :]
    Af = a_buf[idx].view(torch.bfloat16).float()                                 # [Mp][K]
    if case.ln:
        lw = torch.from_numpy(d.ln_w.astype(np.float32))
        lb = torch.from_numpy(d.ln_b.astype(np.float32))
        if mutant == "ln_w_neighbour":
            lw = torch.roll(lw, -1)
        mean = Af.sum(1, keepdim=True) / K
        dlt = Af - mean
        rstd = 1.0 / torch.sqrt((dlt * dlt).sum(1, keepdim=True) / K + 1e-5)
        Af = (((Af * rstd) + (-rstd * mean)) * lw + lb).to(torch.bfloat16).float()
    # ---- split-K slabs, chunk by chunk
    ksl = K // ns
    nch = ksl // 64
    acc = torch.zeros(ns, Mp, Np)
    t0 = min(1, Np // 16 - 1) * 16                                               # the mutated column tile
    for s in range(ns):
        for ch in range(nch):
            k0 = s * ksl + ch * 64
            a = Af[:, k0:k0 + 64]
            part = a @ Wu[:, k0:k0 + 64].t()
            if s == ns - 1 and ch == nch - 1 and mutant == "drop_last_kstep":
                part[:, t0:t0 + 16] = a[:, :32] @ Wu[t0:t0 + 16, k0:k0 + 32].t()
            if s == 0 and ch == 1 and mutant == "stale_chunk":
                part[:, t0:t0 + 16] = Af[:, k0 - 64:k0] @ Wu[t0:t0 + 16, k0:k0 + 64].t()
            acc[s] += part
    # ---- epilogue and stores (flat, so that a stray store lands where the kernel's would)
    flat = out
    n_in = inside_len(case)

    def store(pos, vals):
        """Elements at flat positions `pos` relative to the inside; whatever falls outside the allocation is lost."""
        p = pos.reshape(-1) + G
        ok = (p >= 0) & (p < flat.numel())
        flat[p[ok]] = vals.reshape(-1)[ok]

    ncols16 = (N + 15) // 16 * 16
    if case.mode == 0:
        Nst = Np if mutant == "split_slab_stride" else N
        for s in range(ns):
            ccount = ncols16 if mutant == "tile_past_n_stored" else N
            if mutant == "col_tail_overrun" and N % 4:
                ccount = (N + 3) // 4 * 4
            if first_tile_only:
                ccount = min(16, N)
            mcount = M + 1 if mutant == "row_clamp_stored" else M
            m = torch.arange(mcount)[:, None]
            n = torch.arange(ccount)[None, :]
            vals = _f32_bits(acc[s, :mcount, :ccount])
            # rows in order, the columns past N of a row first: what a later in-range store covers stays covered
            pos = s * M * Nst + m * N + n
            stray = (n >= N) | (m >= M)
            store(pos[stray.expand_as(pos)], vals[stray.expand_as(pos)])
            store(pos[~stray.expand_as(pos)], vals[~stray.expand_as(pos)])
        return
    pre = acc[0]
    if case.mode == 2:
        ccount = ncols16 if mutant == "tile_past_n_stored" else N
        if first_tile_only:
            ccount = min(16, N)
        mcount = M + 1 if mutant == "row_clamp_stored" else M
        m = torch.arange(mcount)[:, None]
        n = torch.arange(ccount)[None, :]
        pos = m * N + n
        src = torch.clamp(m + (1 if mutant == "residual_row_neighbour" else 0), max=M - 1) * N + n
        res = flat[torch.clamp(src + G, max=flat.numel() - 1)].view(torch.bfloat16).float()
        x = (res + pre[:mcount, :ccount].to(torch.bfloat16).float()).to(torch.bfloat16).view(torch.int16)
        stray = ((n >= N) | (m >= M)).expand_as(pos)
        store(pos[stray], x[stray])
        store(pos[~stray], x[~stray])
        return
    # SwiGLU: groups of 16 columns = y[8] | gate[8]
    F = N // 2
    ngrp = Np // 16
    q = pre.to(torch.bfloat16).float().reshape(Mp, ngrp, 2, 8)
    y, gt = q[:, :, 0], q[:, :, 1]
    if mutant == "y_gate_swapped":
        y, gt = gt, y
    if mutant == "swiglu_pair_shift":
        gt = torch.roll(gt, -1, dims=1)
    sl = (gt / (1.0 + torch.exp(-gt))).to(torch.bfloat16).float()
    o = (y * sl).to(torch.bfloat16).view(torch.int16).reshape(Mp, ngrp * 8)
    ccount = Np // 2 if mutant == "tile_past_n_stored" else F
    if first_tile_only:
        ccount = min(8, F)
    mcount = M + 1 if mutant == "row_clamp_stored" else M
    m = torch.arange(mcount)[:, None]
    n = torch.arange(ccount)[None, :]
    pos = m * F + n
    vals = o[:mcount, :ccount]
    stray = ((n >= F) | (m >= M)).expand_as(pos)
    store(pos[stray], vals[stray])
    store(pos[~stray], vals[~stray])
    assert n_in == M * F
