"""Sampler test inputs in which one wrongly kept or dropped token matters, and an fp64 reference (CPU).

On i.i.d. logits the token at the edge of a filter's kept set has a tiny probability and decides the output
about as often. The race noise of both streams is reproducible on the CPU (oracle/philox.py, oracle/
torch_philox.py), so the rows built here put the token that wins the race exactly on a filter boundary:

* **Ladder rows** (top-k, top-p, min-p, unified + min-p, all filters). Rank r has logit -d * T * r (after the
  temperature: a ladder of step d); the ranks are dealt to token ids from the row's noise:
    - the decisive token D, one with very small noise (a lane / register-slot edge token EDGES when its noise
      allows, else the row's arg-min), sits on the last kept rank (variant KEPT: it must win) or on the first
      dropped rank (variant DROPPED: it would win if it were kept);
    - rank 0 goes to W, a token with noise in [W_LO, W_HI] (an edge token when one qualifies), and the other
      ranks above D to tokens with noise >= POOL_LO, so that W is the winner among them by at least
      POOL_LO / W_HI and D, if kept, beats W: noise(D) <= W_LO * exp(-d * ranks) / D_SLACK;
    - every other token takes one of the remaining ranks at random (the filters zero them).
  A filter with k >= V keeps everything: there the ranks follow the noise (rank V-1 = the arg-min) on a flat
  ladder. TIE rows give D, on the first rank beyond k, the logit of rank k-1: equal logits are equal
  probabilities, so the pivot comparison keeps D.
* **Greedy repetition-penalty rows** (temperature 0: nothing is random). A penalised token P (logit x) meets a
  competitor C whose logit lies between two adjacent penalty levels x / rp^c (x * rp^c for x <= 0): variant
  DROPPED (P loses) between the levels count-1 and count, variant KEPT (P wins) between count and count+1.
  The history holds P `count` times inside the window -- once on its first column gen_len - W -- and once
  on the column before it, so one column or one count more or less changes the winner.

**Reference.** reference() restates sample_from_logits (zonos/sampling.py:232-328) in fp64 in the reference's
order and returns per row the token, the race margin (winner's score / runner-up's) and the decision margin
(the smallest relative distance of any token from the threshold that decided it: the exclusive cumsum from
top_p, a probability from the top-k pivot or from min_p * max; greedy rows: the distance of the two largest
penalised logits). `mutant=` switches one deliberate error on (MUTANTS), which is how
tests/test_sampler_probe_cpu.py shows what the rows detect. A row is compared only when its race margin is
at least RACE_MARGIN and its decision margin at least DECISION_MARGIN; a family may leave out at most
MAX_LEFT_OUT of its rows (asserted in families()).

"min-p against the max before the renormalisation of a preceding filter" (min_p_stale_max) keeps the
renormalised p and compares it with min_p times the maximum taken before the last preceding renormalisation
-- what a kernel gets by carrying its max over renorm(). It lowers the threshold by the kept mass, a few ranks
on the all-filters ladder, and is aimed at the DROPPED rows of the call in which min-p binds.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

from oracle import philox, torch_philox

EDGES = (0, 255, 256, 1023, 1024, 1025)      # lane and register-slot edges of the 5-values-per-lane layout
RACE_MARGIN = 1.0 + 2.0 ** -7
DECISION_MARGIN = 2.0 ** -10
MAX_LEFT_OUT = 0.05
W_LO, W_HI, POOL_LO, D_SLACK = 0.3, 0.68, 0.7, 1.05
KEPT, DROPPED, TIE = 0, 1, 2
MAXW = 512                                    # the kernel's window (sampler.hip)

MUTANTS = ("top_k_minus", "top_k_plus", "top_p_inclusive", "top_p_before_temperature", "ent_no_slot4",
           "ent_no_v0", "min_p_stale_max", "win_plus", "win_minus", "win_from_start", "count_once", "no_clamp",
           "mul_positive", "rp_row0", "stride_is_len")

_F32 = np.float32


def f32(x) -> float:
    """The value the kernel receives for a float parameter."""
    return float(_F32(x))


# ---------------------------------------------------------------------------- fp64 reference
def _penalise(x, gen, b, k, K, stride, gen_len, window, rp, mutant):
    """modify_logit_for_repetition_penalty (sampling.py:131-169) on one row."""
    V = x.shape[0]
    off = (b * K + k) * (gen_len if mutant == "stride_is_len" else stride)
    h = gen.reshape(-1)[off:off + gen_len]
    if mutant in ("win_plus", "win_minus", "win_from_start"):
        w = len(h) if window == 0 else min(window, len(h))
        if mutant == "win_from_start":
            h = h[:w]
        else:
            w = min(w + 1, len(h)) if mutant == "win_plus" else max(w - 1, 0)
            h = h[len(h) - w:]
    else:
        h = h[-window:]                                    # sampling.py:142 (-0: is the whole history)
    h = h[h < V] if mutant == "no_clamp" else np.minimum(h, V - 1)      # :143
    cnt = np.bincount(h, minlength=V)
    r = float(rp[0] if mutant == "rp_row0" else rp[b])
    f = np.where(cnt > 0, r, 1.0) if mutant == "count_once" else r ** cnt.astype(np.float64)   # :149, prod
    if mutant == "mul_positive":
        return x * f
    return np.where(x <= 0, x * f, x / f)                  # :169


def _softmax(x):
    e = np.exp(x - x.max())
    return e / e.sum()


def _rel(a, thr):
    """Smallest relative distance of the entries of a from the threshold thr."""
    if a.size == 0 or not thr > 0:
        return math.inf
    return float(np.min(np.abs(a - thr)) / thr)


def _row(x, n, sp, mutant, trace):
    """Everything after the penalty on one row -> (token, race margin, decision margin)."""
    T = f32(sp.get("temperature", 1.0))
    if not T > 0:                                          # sampling.py:325-326
        o = np.argsort(-x, kind="stable")
        a, c = x[o[0]], x[o[1]]
        den = max(abs(a), abs(c))
        return int(o[0]), math.inf, (float((a - c) / den) if den > 0 and np.isfinite(c) else math.inf)
    dec = math.inf
    p = _softmax(x / T)                                    # :298
    stale_max = None                                       # (mutant: the max before the last renormalisation)
    linear, conf, quad = f32(sp.get("linear", 0)), f32(sp.get("conf", 0)), f32(sp.get("quad", 0))
    top_p, top_k, min_p = f32(sp.get("top_p", 0)), int(sp.get("top_k", 0)), f32(sp.get("min_p", 0))
    if linear > 0:                                         # apply_unified :54-75
        lp = np.log(np.maximum(p, 1e-20))
        t = p * lp
        if mutant == "ent_no_slot4":
            t = t[:1024]
        elif mutant == "ent_no_v0":
            t = t[1:]
        ent = -t.sum()
        p = _softmax(lp * (linear + ent * conf) - lp ** 2 * quad)
        trace["entropy"] = ent
    if top_p > 0:                                          # apply_top_p :96-111
        q = _softmax(x) if mutant == "top_p_before_temperature" else p
        o = np.argsort(-q, kind="stable")
        ps = q[o]
        cs = np.cumsum(ps)
        lhs = cs if mutant == "top_p_inclusive" else cs - ps
        drop = lhs > top_p
        dec = min(dec, _rel(lhs[ps > 0], top_p))
        trace["top_p"] = (o, lhs, top_p)
        p = p.copy()
        p[o[drop]] = 0.0
        stale_max = p.max()
        p = p / p.sum()
    if top_k > 0:                                          # apply_top_k :77-93
        kk = top_k + (1 if mutant == "top_k_plus" else -1 if mutant == "top_k_minus" else 0)
        kk = max(min(kk, p.shape[0]), 1)
        pivot = np.sort(p)[::-1][kk - 1]
        dec = min(dec, _rel(p[p != pivot], pivot))
        trace["top_k"] = (p, pivot)
        p = np.where(p < pivot, 0.0, p)
        stale_max = p.max()
        p = p / p.sum()
    if min_p > 0:                                          # apply_min_p :114-128
        thr = min_p * (stale_max if mutant == "min_p_stale_max" and stale_max is not None else p.max())
        dec = min(dec, _rel(p, thr))
        trace["min_p"] = (p, thr)
        p = np.where(p < thr, 0.0, p)
        p = p / p.sum()
    s = p / n                                              # multinomial :26-28
    o = np.argsort(-s, kind="stable")
    trace["score"] = s
    return int(o[0]), (float(s[o[0]] / s[o[1]]) if s[o[1]] > 0 else math.inf), dec


def reference(logits, noise, sp, gen=None, gen_len=0, rp=None, mutant=None, traces=None):
    """fp64 sample_from_logits over one call. logits fp32 [B][K][V]; noise fp32 [B][K][V] (None: greedy);
    sp: the sampler's keyword arguments, window as `repetition_penalty_window`; gen int64 [B][K][stride]
    (None: no history), of which the first gen_len columns are the history; rp fp32 [B].
    -> (tokens int64 [B][K], race margins [B][K], decision margins [B][K])."""
    assert mutant is None or mutant in MUTANTS, mutant
    B, K, V = logits.shape
    tok = np.zeros((B, K), dtype=np.int64)
    race = np.full((B, K), math.inf)
    dec = np.full((B, K), math.inf)
    window = int(sp.get("repetition_penalty_window", 2))
    penal = gen is not None and rp is not None and bool((np.asarray(rp, dtype=_F32) != 1).any())   # :284
    for b in range(B):
        for k in range(K):
            x = logits[b, k].astype(np.float64)
            if penal:
                x = _penalise(x, gen, b, k, K, gen.shape[2], gen_len, window, np.asarray(rp, dtype=_F32), mutant)
            tr = {}
            tok[b, k], race[b, k], dec[b, k] = _row(x, None if noise is None else noise[b, k].astype(np.float64),
                                                    sp, mutant, tr)
            if traces is not None:
                traces.append(tr)
    return tok, race, dec


# ---------------------------------------------------------------------------- ladder rows
def _pick(cands, ok, rot):
    """The first of cands (rotated by rot) for which ok holds, else None."""
    n = len(cands)
    for i in range(n):
        c = cands[(rot + i) % n]
        if ok(c):
            return c
    return None


def ladder_row(noise, nkept, d, T, variant, rng, rot=0, by_noise=False, top_edges=False, race_d=None, plateau=None,
               forbid=()):
    """Logits fp32 [V] for one row whose reference keeps the ranks 0 .. nkept-1 -> (logits, D, W); (None,) * 3
    when the noise row cannot host the construction (the row is then left out). race_d: the step of the
    log-probabilities the race sees, where a reshaping (unified) stretches the ladder. plateau: the ranks from
    it on share one logit (few distinct values: bf16-exact slabs). forbid: tokens that take no role (they get
    one of the remaining ranks)."""
    V = noise.shape[0]
    lad = (-(d * T) * np.minimum(np.arange(V), plateau or V)).astype(_F32)
    if len(forbid):
        noise = noise.copy()
        noise[list(forbid)] = 0.5 * (W_HI + POOL_LO)      # neither D, nor W, nor in the pool
    if by_noise:                                   # everything is kept: the ranks follow the noise
        order = np.argsort(-noise, kind="stable")
        logits = np.empty(V, dtype=_F32)
        logits[order] = lad
        return logits, int(order[-1]), int(order[-1])
    rD = nkept - 1 if variant == KEPT else nkept   # D's rank = the number of tokens above it
    edges = [e for e in EDGES if e < V and e not in forbid] + ([V - 1] if V - 1 not in EDGES else [])
    qD = W_LO * math.exp(-(race_d or d) * rD) / D_SLACK
    D = _pick(edges, lambda e: noise[e] <= qD, rot)
    if D is None:
        D = int(np.argmin(noise))
        if noise[D] > qD:
            return None, None, None
    above = []
    if rD >= 1:
        W = _pick(edges, lambda e: e != D and W_LO <= noise[e] <= W_HI, rot // len(edges))
        if W is None:
            c = np.flatnonzero((noise >= W_LO) & (noise <= W_HI))
            c = c[c != D]
            if c.size == 0:
                return None, None, None
            W = int(c[rng.integers(c.size)])
        pool = np.flatnonzero(noise >= POOL_LO)
        pool = pool[(pool != D) & (pool != W)]
        if pool.size < rD - 1:
            return None, None, None
        pool = rng.permutation(pool)
        if top_edges:                              # edge tokens take the ranks next to the top (entropy rows)
            pool = np.concatenate([pool[np.isin(pool, edges)], pool[~np.isin(pool, edges)]])
        above = [W] + [int(t) for t in pool[:rD - 1]]
    else:
        W = None
    taken = np.zeros(V, dtype=bool)
    taken[above + [D]] = True
    rest = rng.permutation(np.flatnonzero(~taken))
    order = np.concatenate([np.array(above + [D], dtype=np.int64), rest])
    logits = np.empty(V, dtype=_F32)
    logits[order] = lad
    if variant == TIE:
        logits[D] = lad[rD - 1]
    return logits, D, (D if variant in (KEPT, TIE) else W)


# ---------------------------------------------------------------------------- cases
@dataclass
class Case:
    family: str
    name: str
    sp: dict                          # sampler keyword arguments
    logits: np.ndarray                # fp32 [B][K][V]
    noise: np.ndarray | None          # fp32 [B][K][V]
    variant: np.ndarray               # [B][K] KEPT / DROPPED / TIE, -1: the row could not be built
    decisive: np.ndarray              # [B][K] the token on the boundary
    coords: dict = field(default_factory=dict)      # keyed: seed, step, draw, row_base
    gen: np.ndarray | None = None     # int64 [B][K][stride]
    gen_len: int = 0
    rp: np.ndarray | None = None      # fp32 [B]
    direct: bool = False              # needs the C entry (gen_stride > gen_len)
    tags: np.ndarray | None = None    # [B][K] what a greedy row covers
    tok: np.ndarray | None = None     # finish(): the reference's tokens, margins and the rows that are compared
    race: np.ndarray | None = None
    dec: np.ndarray | None = None
    use: np.ndarray | None = None

    def finish(self):
        self.tok, self.race, self.dec = reference(self.logits, self.noise, self.sp, self.gen, self.gen_len, self.rp)
        self.use = (self.variant >= 0) & (self.race >= RACE_MARGIN) & (self.dec >= DECISION_MARGIN)
        # a built row answers as designed: D wins where it is kept, and does not where it is dropped
        u = self.use
        assert np.array_equal(self.tok[u & (self.variant != DROPPED)], self.decisive[u & (self.variant != DROPPED)]), \
            self.name
        assert not (self.tok[u & (self.variant == DROPPED)] == self.decisive[u & (self.variant == DROPPED)]).any(), \
            self.name
        return self

    def mutant_tokens(self, mutant):
        return reference(self.logits, self.noise, self.sp, self.gen, self.gen_len, self.rp, mutant=mutant)[0]

    @property
    def shape(self):
        return self.logits.shape


def keyed_noise(c: dict, B, K, V):
    return philox.exp_noise(c["seed"], c["step"], c["draw"], B, K, V, row_base=c["row_base"])


def torch_noise(seed, offset, stride, B, K, V):
    return torch_philox.exp_noise(B * K * V, seed, offset, stride).reshape(B, K, V)


def _probs_of_ladder(V, d):
    p = np.exp(-d * np.arange(V, dtype=np.float64))
    return p / p.sum()


def ladder_case(family, name, noise, coords, nkept, d, sp, T=1.0, tie=False, by_noise=False, top_edges=False,
                race_d=None, plateau=None, forbid=(), seed=0):
    """One call of ladder rows; the rows alternate KEPT / DROPPED (by_noise: KEPT, tie: TIE)."""
    B, K, V = noise.shape
    rng = np.random.default_rng([seed, nkept, V])
    logits = np.zeros((B, K, V), dtype=_F32)
    variant = np.full((B, K), -1, dtype=np.int64)
    D = np.zeros((B, K), dtype=np.int64)
    for b in range(B):
        for k in range(K):
            i = b * K + k
            var = TIE if tie else KEPT if by_noise or nkept >= V else (KEPT, DROPPED)[i % 2]
            lg, d_, _ = ladder_row(noise[b, k], nkept, d, T, var, rng, rot=i // 2 + seed, by_noise=by_noise,
                                   top_edges=top_edges, race_d=race_d, plateau=plateau, forbid=forbid)
            if lg is None:
                continue
            logits[b, k], variant[b, k], D[b, k] = lg, var, d_
    sp = dict(temperature=T, **sp)
    return Case(family, name, sp, logits, noise, variant, D, coords).finish()


def _top_p_between(V, d, nkept):
    """top_p halfway between the exclusive cumsums of the ranks nkept-1 (kept) and nkept (dropped)."""
    cs = np.cumsum(_probs_of_ladder(V, d))
    return f32(0.5 * (cs[nkept - 2] + cs[nkept - 1]))


def _min_p_between(d, nkept):
    """min_p halfway, in log space, between the ranks nkept-1 and nkept of a ladder of step d."""
    return f32(math.exp(-d * (nkept - 0.5)))


def _unified_min_p(V, d, nkept, linear, conf, quad):
    """(min_p halfway, in log space, between the ranks nkept-1 and nkept after apply_unified, the mean step of
    the reshaped ladder down to rank nkept)."""
    p = _probs_of_ladder(V, d)
    lp = np.log(p)
    raw = lp * (f32(linear) + -(p * lp).sum() * f32(conf)) - lp ** 2 * f32(quad)
    return f32(math.exp(0.5 * (raw[nkept - 1] + raw[nkept]) - raw[0])), float(raw[0] - raw[nkept]) / nkept


# (the ladder specs: family, name, V, builder of (nkept, d, sp, extras); every spec is one call per step)
def _ladder_specs():
    S = []
    V = 1026
    for k in (1, 2, 20):
        S.append(("top_k", f"k{k}", V, dict(nkept=k, d=0.0625, sp=dict(top_k=k))))
    for k in (V, V + 5):
        S.append(("top_k", f"k{k}", V, dict(nkept=V, d=2.0 ** -9, sp=dict(top_k=k), by_noise=True)))
    S.append(("top_k", "k20-tie", V, dict(nkept=20, d=0.0625, sp=dict(top_k=20), tie=True)))
    for v in (257, 1280):
        S.append(("top_k", f"k20-V{v}", v, dict(nkept=20, d=0.0625, sp=dict(top_k=20))))
    for nk, T in ((12, 1.0), (16, 0.7), (6, 1.0), (14, 1.3)):
        S.append(("top_p", f"n{nk}-T{T}", V, dict(nkept=nk, d=0.1, T=T, sp=dict(top_p=_top_p_between(V, 0.1, nk)))))
    for v, T in ((257, 0.8), (1280, 1.0)):         # (temperature != 1 in half of the family's calls)
        S.append(("top_p", f"n12-V{v}-T{T}", v, dict(nkept=12, d=0.1, T=T, sp=dict(top_p=_top_p_between(v, 0.1, 12)))))
    for nk, d in ((2, 0.25), (17, 0.0625), (40, 0.03125)):
        S.append(("min_p", f"n{nk}", V, dict(nkept=nk, d=d, sp=dict(min_p=_min_p_between(d, nk)))))
    for nk, (lin, conf, quad) in ((300, (0.55, 0.4, 0.0)), (200, (0.55, 0.4, 0.002)), (300, (1.2, -0.06, 0.0)),
                                  (120, (0.3, 0.2, 0.004))):
        d = 2.0 ** -8
        mp, rd = _unified_min_p(V, d, nk, lin, conf, quad)
        S.append(("unified_min_p", f"n{nk}-l{lin}-c{conf}-q{quad}", V,
                  dict(nkept=nk, d=d, top_edges=True, race_d=rd, sp=dict(linear=lin, conf=conf, quad=quad, min_p=mp))))
    d = 0.1                            # all filters on: each binds in turn, the others keep a few ranks more
    S.append(("all_filters", "top_k-binds", V,
              dict(nkept=10, d=d, sp=dict(top_p=_top_p_between(V, d, 16), top_k=10, min_p=_min_p_between(d, 14)))))
    S.append(("all_filters", "top_p-binds", V,
              dict(nkept=9, d=d, sp=dict(top_p=_top_p_between(V, d, 9), top_k=14, min_p=_min_p_between(d, 12)))))
    S.append(("all_filters", "min_p-binds", V,
              dict(nkept=8, d=d, sp=dict(top_p=_top_p_between(V, d, 15), top_k=12, min_p=_min_p_between(d, 8)))))
    return S


B_DEF, K_DEF = 8, 9
KEYED_SEED = 0x5A4D504C45520001
KEYED_STEPS = ((1, 0, 0), (7, 1, 3), (3001, 0, 5), (640, 1, 16))     # (step, draw, row_base) of a spec's calls


def keyed_ladder_cases(families=None, steps=KEYED_STEPS):
    """Every ladder spec at every (step, draw, row_base) of `steps`, on the keyed stream."""
    out = []
    for i, (fam, name, V, kw) in enumerate(_ladder_specs()):
        if families is not None and fam not in families:
            continue
        for j, (step, draw, rb) in enumerate(steps):
            co = dict(seed=KEYED_SEED + i, step=step + i, draw=draw, row_base=rb)
            out.append(ladder_case(fam, f"{name}-s{co['step']}", keyed_noise(co, B_DEF, K_DEF, V), co, seed=j, **kw))
    return out


def torch_ladder_cases(stride_of, seed, offset0, families=("top_k", "top_p", "unified_min_p")):
    """The ladder specs of `families` on torch's stream: one call each, at consecutive Philox offsets from
    offset0 as torch's generator would hand them out. stride_of(n) -> (stride, incr) is the device's policy.
    -> [(case, offset, stride, incr)]."""
    out, off = [], offset0
    for fam, name, V, kw in _ladder_specs():
        if fam not in families:
            continue
        stride, incr = stride_of(B_DEF * K_DEF * V)
        noise = torch_noise(seed, off, stride, B_DEF, K_DEF, V)
        out.append((ladder_case(fam, f"{name}-o{off}", noise, dict(seed=seed, offset=off, stride=stride), **kw),
                    off, stride, incr))
        off += incr
    return out


# ---------------------------------------------------------------------------- greedy repetition-penalty rows
def _level(x, rp, c):
    return x * rp ** c if x <= 0 else x / rp ** c


def greedy_case(name, V, window, gen_len, stride, rps, xs, quantum=None, seed=0, counts=(1, 2, 3), high_tokens=False,
                coords=None, B=B_DEF, K=K_DEF, forbid=(), unique_tokens=False):
    """One call of greedy rows. Row i: count = counts[i % len], x = xs[(i // 3) % len], variant i % 2
    (DROPPED: P loses, KEPT: P wins), rp = rps[b]. The history: P on the first column of the window, on
    count - 1 further columns inside it and on the column before it; every other column holds a filler token
    whose logit is far below. Columns gen_len .. stride-1 hold P (reading them over-penalises it).
    quantum: logits are multiples of it (bf16-exact slabs for the heads kernel). high_tokens (V < 1026): the
    history holds 1024 / 1025 instead of P = V-1, which the clamp maps onto it. forbid: tokens that take no
    role (the heads kernel masks 1025 and biases EOS). unique_tokens: every row has a P and a C of its own, so a
    history read at another row's place never holds them."""
    rng = np.random.default_rng([seed, V, window, gen_len])
    W = gen_len if window == 0 else min(window, gen_len)
    assert W <= MAXW
    q = quantum or 2.0 ** -6
    logits = (-96.0 - 4.0 * rng.integers(0, 7, size=(B, K, V))).astype(_F32)     # far below every level
    gen = np.zeros((B, K, max(stride, 1)), dtype=np.int64)
    variant = np.full((B, K), -1, dtype=np.int64)
    Ptok = np.zeros((B, K), dtype=np.int64)
    tags = np.empty((B, K), dtype=object)
    edges = [e for e in EDGES if e < V and e not in forbid]
    rp = np.asarray(rps, dtype=_F32)[:B]
    for b in range(B):
        for k in range(K):
            i = b * K + k
            x = float(xs[(i // 3) % len(xs)])
            cnt = counts[i % len(counts)]
            var = (DROPPED, KEPT)[i % 2]
            P = V - 1 if high_tokens else edges[i % len(edges)]
            C = edges[(i + 1 + i // len(edges)) % len(edges)]
            if C == P:
                C = edges[(i + 2) % len(edges)]
            if unique_tokens:
                P, C = 300 + i, 400 + i
            filler = [t for t in range(7, 7 + 8) if t not in (P, C)]
            hist = rng.choice(filler, size=stride)
            inside = min(cnt, W)
            if W > 0:
                cols = [gen_len - W] + list(gen_len - W + 1 + rng.permutation(W - 1)[:inside - 1])
                for j, col in enumerate(cols):
                    hist[col] = (1024 + j % 2) if high_tokens else P
                inside = len(cols)
            if gen_len - W - 1 >= 0:
                hist[gen_len - W - 1] = 1024 if high_tokens else P
            hist[gen_len:] = P
            gen[b, k, :stride] = hist
            r = float(rp[b])
            eff = inside if r != 1.0 else 0
            if x == 0.0 or r == 1.0:                      # no level moves: C sits just below / above P
                c = x - 0.5 if var == KEPT else x + 0.5
            else:
                lo = _level(x, r, eff + (0.5 if var == KEPT else -0.5))
                c = round(lo / q) * q
            logits[b, k, P], logits[b, k, C] = x, c
            variant[b, k], Ptok[b, k] = var, P
            tags[b, k] = (inside, "zero" if x == 0 else "neg" if x < 0 else "pos", r)
    sp = dict(temperature=0.0, repetition_penalty_window=window)
    case = Case("greedy_rp", name, sp, logits, None, variant, Ptok, coords or dict(seed=1, step=0, draw=0, row_base=0),
                gen if stride > 0 else None, gen_len, rp, direct=stride != gen_len or gen_len == 0, tags=tags)
    return case.finish()


RPS = (1.25, 2.0, 3.0, 2.25, 1.0, 2.5, 2.0, 1.75)
XS = (8.0, -1.0, 0.0, 4.0, -0.5)


def greedy_cases():
    """The greedy family: the window's first column and the one before it, counts 1-3, logits <= 0, > 0 and 0,
    per-row rp (one row rp = 1), gen_len < W, gen_len = 0, gen_stride > gen_len, history tokens >= V, and the
    reference's slice at window 0 and at a window beyond the history."""
    return [greedy_case("W8-len19", 1026, 8, 19, 19, RPS, XS),
            greedy_case("W8-len5", 1026, 8, 5, 5, RPS, XS, seed=1),
            greedy_case("W8-len0", 1026, 8, 0, 4, RPS, XS, seed=2),
            greedy_case("W8-len19-stride40", 1026, 8, 19, 40, RPS, XS, seed=3, unique_tokens=True),
            greedy_case("W8-len19-V1000", 1000, 8, 19, 19, RPS, (8.0, -1.0, 4.0), seed=4, high_tokens=True),
            greedy_case("W0-len12", 1026, 0, 12, 12, RPS, XS, seed=5),
            greedy_case("W0-len300", 1026, 0, 300, 300, RPS, XS, seed=6),
            greedy_case("W600-len20", 1026, 600, 20, 20, RPS, XS, seed=7),
            greedy_case("W512-len700", 1026, 512, 700, 700, RPS, XS, seed=8),
            greedy_case("W1-len3", 1026, 1, 3, 3, RPS, XS, seed=9, counts=(1,))]


# ---------------------------------------------------------------------------- rows for the engine sampler
EOS, MASK = 1024, 1025
LOG1024F = _F32(6.931471824645996)              # float32(log(1024)) (model.py:324)
HEADS_FORBID = (EOS, MASK)


def heads_logits(combined, prefill=False, act=None, new_eos=None, force_full_length=False):
    """What k_sample_heads samples from, given the CFG-combined logits fp32 [B][K][V]: tokens >= 1025 masked
    (model.py:115) and the EOS column rules (model.py:322-324, 353, 360-361, 387), in fp32 as the reference."""
    x = combined.copy()
    x[..., MASK:] = -np.inf
    if not prefill:
        x[:, 1:, EOS] = -np.inf
        x[:, 0, EOS] = x[:, 0, EOS] - LOG1024F
        for rows in (act, new_eos):
            if rows is not None:
                x[np.asarray(rows, dtype=bool), 0, EOS] = -np.inf
    if force_full_length:
        x[:, 0, EOS] = -np.inf
    return x


def heads_slabs(combined, nsplit, cfg_scale, rng):
    """Split-K slabs fp32 [nsplit][2B][K * V] that the kernel CFG-combines to `combined` exactly: u holds
    multiples of 1/2 in [-4, 4] and c = u + (combined - u) / cfg_scale; asserted here: c and u are bf16 values
    (so the rounding of the head outputs, model.py:111, changes nothing), the slabs (multiples of 2^-6) sum to
    them exactly in fp32, and u + (c - u) * cfg_scale is `combined` in fp32."""
    import torch
    B, K, V = combined.shape
    u = 0.5 * rng.integers(-8, 9, size=(B, K, V))
    c = u + (combined.astype(np.float64) - u) / cfg_scale
    full = np.concatenate([c, u]).reshape(2 * B, K * V)
    assert np.array_equal(torch.from_numpy(full).to(torch.bfloat16).double().numpy(), full)
    parts = [2.0 ** -6 * rng.integers(-256, 257, size=full.shape) for _ in range(nsplit - 1)]
    parts.append(full - sum(parts))
    slabs = np.stack(parts).astype(_F32)
    acc = np.zeros_like(slabs[0])
    for p in slabs:
        acc = acc + p
    assert np.array_equal(acc.astype(np.float64), full)
    c32, u32 = acc[:B].reshape(B, K, V), acc[B:].reshape(B, K, V)
    assert np.array_equal(u32 + (c32 - u32) * _F32(cfg_scale), combined)
    return slabs


# ---------------------------------------------------------------------------- families and their left-out shares
_CACHE = {}


def families():
    """{family: [Case]} on the keyed stream, built once. Asserts the left-out share of every family."""
    if "fam" not in _CACHE:
        fam = {}
        for c in keyed_ladder_cases() + greedy_cases():
            fam.setdefault(c.family, []).append(c)
        for name, cases in fam.items():
            share = left_out(cases)
            assert share <= MAX_LEFT_OUT, f"{name}: {share:.3f} of the candidate rows left out"
        _CACHE["fam"] = fam
    return _CACHE["fam"]


def left_out(cases) -> float:
    n = sum(c.use.size for c in cases)
    return 1.0 - sum(int(c.use.sum()) for c in cases) / n


def edge_coverage(cases):
    """(decisive tokens, expected winners of DROPPED rows) over the used rows."""
    dec, win = set(), set()
    for c in cases:
        dec.update(c.decisive[c.use].tolist())
        win.update(c.tok[c.use & (c.variant == DROPPED)].tolist())
    return dec, win
