"""CPU: what the sampler edge rows (tests/sampler_probe.py) establish before a GPU sees them.

* the fp32 oracle (oracle/zonos_ref.sample) returns the fp64 reference's token on every used row;
* the fp32 oracle's race scores and filter-threshold comparisons deviate from the fp64 reference by at most
  one eighth of the margins the rows were selected with, so an fp32 kernel in the reference's order has room;
* each deliberate error of the reference (sampler_probe.MUTANTS) changes the token of the rows aimed at it;
* the reference's slice semantics at window 0 and at a window beyond the history.
The figures are printed (pytest -s) and recorded in profiles/sampler_edge_tests.txt."""
import numpy as np
import pytest
import torch

from oracle import zonos_ref as zr

from . import sampler_probe as sp
from .sampler_probe import DROPPED, KEPT


@pytest.fixture(scope="module")
def fam():
    return sp.families()


def _oracle(case, decision=None):
    """The fp32 oracle's tokens [B][K] of one call."""
    kw = dict(case.sp)
    gen = None if case.gen is None else torch.from_numpy(case.gen[..., :case.gen_len])
    rp = 1.0 if case.rp is None else torch.from_numpy(case.rp)
    noise = None if case.noise is None else torch.from_numpy(case.noise)
    return zr.sample(torch.from_numpy(case.logits), noise, generated_tokens=gen, repetition_penalty=rp,
                     decision=decision, **kw).squeeze(-1).numpy()


def test_left_out_shares_and_edges(fam):
    for name, cases in fam.items():
        share = sp.left_out(cases)
        rows = sum(c.use.size for c in cases)
        print(f"{name}: {rows} candidate rows, {share * 100:.2f} % left out")
        assert share <= sp.MAX_LEFT_OUT
        dec, win = sp.edge_coverage(cases)
        assert set(sp.EDGES) <= dec, (name, sorted(set(sp.EDGES) - dec))
        assert set(sp.EDGES) <= win, (name, sorted(set(sp.EDGES) - win))
    for fam_name in ("top_k", "top_p"):                 # V = 257 (two slots, one padded) and V = 1280 (none padded)
        for V, edges in ((257, {0, 255, 256}), (1280, set(sp.EDGES) | {1279})):
            dec, win = sp.edge_coverage([c for c in fam[fam_name] if c.shape[2] == V])
            assert edges <= dec and edges <= win, (fam_name, V, sorted(edges - dec), sorted(edges - win))


def test_fp32_oracle_agrees(fam):
    for name, cases in fam.items():
        flips = rows = 0
        for c in cases:
            tok = _oracle(c)
            flips += int((tok != c.tok)[c.use].sum())
            rows += int(c.use.sum())
        print(f"{name}: fp32 oracle flips {flips} of {rows}")
        assert flips == 0, name


def _stage_deviation(case):
    """Largest relative deviation of the fp32 oracle from the fp64 reference over the used rows of one call:
    (race scores of the winner and the runner-up, filter-threshold comparisons). A comparison's two sides are
    taken relative to the threshold, for every token within a factor 2 of it."""
    B, K, V = case.shape
    traces, decision = [], []
    sp.reference(case.logits, case.noise, case.sp, case.gen, case.gen_len, case.rp, traces=traces)
    _oracle(case, decision)
    s32 = decision[0][1].double().numpy()
    kw = case.sp
    race = thr = 0.0
    p32 = torch.softmax(torch.from_numpy(case.logits) / kw["temperature"], dim=-1)
    if kw.get("linear", 0) > 0:
        p32 = zr.shape_probs(p32, linear=kw["linear"], conf=kw["conf"], quad=kw["quad"])
    stage = {}
    if kw.get("top_p", 0) > 0:
        ps, pi = torch.sort(p32, dim=-1, descending=True)
        stage["top_p"] = torch.zeros_like(p32).scatter(-1, pi, torch.cumsum(ps, dim=-1) - ps).double().numpy()
        p32 = zr.shape_probs(p32, top_p=kw["top_p"])
    if kw.get("top_k", 0) > 0:
        piv = torch.topk(p32, min(kw["top_k"], V))[0][..., -1:]
        stage["top_k"] = (p32.double().numpy(), piv.double().numpy())
        p32 = zr.shape_probs(p32, top_k=kw["top_k"])
    if kw.get("min_p", 0) > 0:
        t = kw["min_p"] * p32.max(dim=-1, keepdim=True)[0]
        stage["min_p"] = (p32.double().numpy(), t.double().numpy())
    for b in range(B):
        for k in range(K):
            if not case.use[b, k]:
                continue
            tr = traces[b * K + k]
            top2 = np.argsort(-tr["score"], kind="stable")[:2]
            top2 = top2[tr["score"][top2] > 0]
            race = max(race, float(np.max(np.abs(s32[b, k, top2] / tr["score"][top2] - 1.0))))
            if "top_p" in tr:
                o, lhs, t = tr["top_p"]
                near = (lhs >= t / 2) & (lhs <= 2 * t)
                thr = max(thr, float(np.max(np.abs(stage["top_p"][b, k][o[near]] - lhs[near]) / t)))
            for key in ("top_k", "min_p"):
                if key in tr:
                    p64, t = tr[key]
                    q32, t32 = stage[key]
                    if not t > 0:                # (top-k after a top-p that left fewer than k: nothing decided)
                        continue
                    near = (p64 >= t / 2) & (p64 <= 2 * t)
                    thr = max(thr, float(np.max(np.abs(q32[b, k][near] / t32[b, k] - p64[near] / t))))
    return race, thr


def test_fp32_deviation_is_an_eighth_of_the_margins(fam):
    race = thr = 0.0
    for name, cases in fam.items():
        if name == "greedy_rp":              # temperature 0: one comparison of two logits, checked below
            continue
        fr = ft = 0.0
        for c in cases:
            r, t = _stage_deviation(c)
            fr, ft = max(fr, r), max(ft, t)
        print(f"{name}: fp32 oracle deviation, race scores {fr:.3e}, threshold comparisons {ft:.3e}")
        race, thr = max(race, fr), max(thr, ft)
    print(f"largest: race {race:.3e} (margin / 8 = {(sp.RACE_MARGIN - 1) / 8:.3e}), "
          f"thresholds {thr:.3e} (margin / 8 = {sp.DECISION_MARGIN / 8:.3e})")
    assert race <= (sp.RACE_MARGIN - 1) / 8
    assert thr <= sp.DECISION_MARGIN / 8
    # greedy rows: the fp32 penalised logits of the two leaders against the fp64 ones
    g = 0.0
    for c in fam["greedy_rp"]:
        decision, traces = [], []
        _oracle(c, decision)
        x32 = decision[0][1].double().numpy()
        B, K, V = c.shape
        for b in range(B):
            for k in range(K):
                x = c.logits[b, k].astype(np.float64)
                if c.gen is not None:
                    x = sp._penalise(x, c.gen, b, k, K, c.gen.shape[2], c.gen_len,
                                     c.sp["repetition_penalty_window"], c.rp, None)
                top2 = np.argsort(-x, kind="stable")[:2]
                den = np.max(np.abs(x[top2]))
                g = max(g, float(np.max(np.abs(x32[b, k, top2] - x[top2])) / den))
    print(f"greedy_rp: fp32 oracle deviation of the two leading penalised logits {g:.3e}")
    assert g <= sp.DECISION_MARGIN / 8


def _tag_mask(c, fn):
    return np.array([[fn(*c.tags[b, k]) for k in range(c.shape[1])] for b in range(c.shape[0])])


def _greedy(variant, outside=False, min_inside=1, kind=None, b_from=0, only=None):
    """Rows of the greedy family a penalty mutant is aimed at: rp != 1, logit != 0, the given variant."""
    def rows(c):
        if only is not None and not c.name.startswith(only):
            return None
        W = c.gen_len if c.sp["repetition_penalty_window"] == 0 else min(c.sp["repetition_penalty_window"], c.gen_len)
        if W == 0 or (outside and c.gen_len <= W):
            return None
        m = _tag_mask(c, lambda inside, knd, r: r != 1.0 and knd != "zero" and inside >= min_inside and
                      (kind is None or knd == kind))
        m &= c.variant == variant
        m[:b_from] = False
        return m
    return rows


def _ladder(variant, pred=lambda c: True):
    return lambda c: (c.variant == variant) if pred(c) else None


# mutant -> (family, rows aimed at, exempt from the 90 % (moves a boundary only slightly))
TARGETS = {
    "top_k_minus": ("top_k", _ladder(KEPT, lambda c: 2 <= c.sp["top_k"] <= c.shape[2]), False),
    "top_k_plus": ("top_k", _ladder(DROPPED), False),
    "top_p_inclusive": ("top_p", _ladder(KEPT), False),
    "top_p_before_temperature": ("top_p", lambda c: None if c.sp["temperature"] == 1.0 else
                                 c.variant == (DROPPED if c.sp["temperature"] < 1 else KEPT), False),
    "ent_no_slot4": ("unified_min_p", lambda c: c.variant >= 0, True),
    "ent_no_v0": ("unified_min_p", lambda c: c.variant >= 0, True),
    "min_p_stale_max": ("all_filters", _ladder(DROPPED, lambda c: c.name.startswith("min_p-binds")), False),
    "win_plus": ("greedy_rp", _greedy(KEPT, outside=True), False),
    "win_minus": ("greedy_rp", _greedy(DROPPED), False),
    "win_from_start": ("greedy_rp", _greedy(DROPPED, only="W8-len19"), False),
    "count_once": ("greedy_rp", _greedy(DROPPED, min_inside=2), False),
    "no_clamp": ("greedy_rp", _greedy(DROPPED, only="W8-len19-V1000"), False),
    "mul_positive": ("greedy_rp", _greedy(DROPPED, kind="pos"), False),
    "rp_row0": ("greedy_rp", _greedy(DROPPED, b_from=1), False),
    "stride_is_len": ("greedy_rp", _greedy(DROPPED, only="W8-len19-stride40", b_from=1), False),
}


@pytest.mark.parametrize("mutant", sp.MUTANTS)
def test_mutant_changes_the_token(fam, mutant):
    family, rows_of, exempt = TARGETS[mutant]
    flipped = rows = 0
    for c in fam[family]:
        m = rows_of(c)
        if m is None:
            continue
        m = m & c.use
        if not m.any():
            continue
        tok = c.mutant_tokens(mutant)
        flipped += int((tok != c.tok)[m].sum())
        rows += int(m.sum())
    print(f"{mutant}: flips {flipped} of {rows} rows aimed at it ({100.0 * flipped / max(rows, 1):.1f} %)")
    assert flipped >= 10
    if not exempt:
        assert flipped >= 0.9 * rows


def test_window_slices_are_the_references():
    """generated[..., -window:] (sampling.py:142): a window of 0 and a window beyond the history both penalise
    the whole history. Tokens 3, 3, 5 with rp 2: the whole history leaves 8 / 4, 3 / 2 and token 1's 2.5."""
    logits = np.full((1, 1, 8), -5.0, dtype=np.float32)
    logits[0, 0, [1, 3, 5]] = (2.5, 8.0, 3.0)
    gen = np.array([[[3, 3, 5]]], dtype=np.int64)
    rp = np.array([2.0], dtype=np.float32)
    for window, want in ((0, 1), (10, 1), (3, 1), (2, 3), (1, 3)):
        kw = dict(temperature=0.0, repetition_penalty_window=window)
        tok = sp.reference(logits, None, kw, gen, 3, rp)[0]
        assert int(tok[0, 0]) == want, (window, tok)
        ora = zr.sample(torch.from_numpy(logits), None, generated_tokens=torch.from_numpy(gen),
                        repetition_penalty=torch.from_numpy(rp), **kw)
        assert int(ora[0, 0, 0]) == want, (window, ora)


def test_generate_refuses_windows_the_sampler_cannot_take():
    """HipDecoder.generate and the hybrid engine (the same generate) check their sampling parameters with
    check_sampling_params: window 0 (the reference's whole history) and windows beyond the kernel's 512."""
    from zonos_amd import engine, hybrid
    assert hybrid.HybridDecoder.generate is engine.HipDecoder.generate
    for window in (1, 2, 8, 512):
        engine.check_sampling_params(dict(repetition_penalty_window=window))
    for window in (0, -1, 513, 100000):
        with pytest.raises(ValueError, match="repetition_penalty_window"):
            engine.check_sampling_params(dict(repetition_penalty_window=window))
