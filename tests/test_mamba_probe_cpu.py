"""CPU: what the Mamba probe cases (tests/mamba_probe.py) establish before a GPU sees them.

* every case has the properties its docstring claims (slow / fast / threshold heads, one-hot B and C on the
  probe row, impulses, distinct taps, index separation);
* the clean fp32 restatement stays within the derived bound -- final SSM state, yz of every step, the norm
  output -- in every mode (prefill, step chain, prefill then steps), also with the fp32 term halved (the rule
  the term is chosen by), and its conv states equal the reference's bit for bit;
* every mutant exceeds the bound on every case aimed at it;
* the i.i.d. one-step data of test_gpu_hybrid.py::test_mamba_step_kernel_vs_oracle do not catch a dropped
  state-element update under that test's assertions.
The figures are printed (pytest -s) and recorded in profiles/mamba_probe_tests.txt."""
import numpy as np
import pytest

from . import mamba_probe as mp

S0_MIXED = (1, 3, 16, 17)


@pytest.fixture(scope="module")
def cases():
    return mp.cases()


def modes(S):
    """S0 of every mode a case is run in: prefill (S), step chain (0), prefill(S0) then steps."""
    return [S, 0] + [s for s in S0_MIXED if s < S]


def worst(case, S0, got, f32_term=mp.F32_TERM):
    """What the GPU tests assert of a result, as one figure (<= 1 passes): the ratios of xc, of the final state, of
    yz and of the norm output to their bounds, inf for a conv state that differs (after a prefill only its last
    state exists). Where xc is within its bound (one ulp, where a flip is possible at all) the state, yz and the
    norm output are also measured against the reference recurrence fed with the result's own xc, as the prefill
    test does."""
    S = case.S
    ref = case.ref(S0, f32_term)
    first = max(S0 - 1, 0)
    r = [mp.ratio(got["ssm"], ref.ssm, ref.e_ssm), mp.ratio(got["yz"], ref.yz, ref.e_yz),
         mp.ratio(got["out"], ref.out, ref.e_out), mp.ratio(got["xc"], ref.xc, ref.e_xc),
         0.0 if np.array_equal(got["conv"][:, first:], ref.conv[:, first:]) else np.inf]
    if max(r) <= 1:
        own = mp.reference(case.zx, case.P, round_at=mp.round_points(S, S0), xc=got["xc"], f32_term=f32_term)
        r += [mp.ratio(got["ssm"], own.ssm, own.e_ssm), mp.ratio(got["yz"], own.yz, own.e_yz),
              mp.ratio(got["out"], own.out, own.e_out)]
    return max(r)


def loose(case, S0, got):
    """The same against the loose bound (a flip allowed at every rounding point): finite figures to print."""
    ref = case.ref(S0, sharp=False)
    return max(mp.ratio(got[k], getattr(ref, k), getattr(ref, "e_" + k)) for k in ("xc", "ssm", "yz", "out"))


def test_cases_have_their_properties(cases):
    for c in cases.values():
        mp.check_properties(c)
    assert len(cases) == len(mp.GEOMS) * len(mp.LENGTHS)


def test_clean_restatement_is_within_the_bound(cases):
    """Also with half the fp32 term: the restatement may use at most half of it (mamba_probe docstring)."""
    flips = total = 0
    for hp, ds in mp.GEOMS:
        full = half = lo = 0.0
        for S in mp.LENGTHS:
            c = cases[hp, ds, S]
            for S0 in modes(S):
                got = mp.emulate(c.zx, c.P, S0)
                full = max(full, worst(c, S0, got))
                half = max(half, worst(c, S0, got, f32_term=mp.F32_TERM / 2))
                lo = max(lo, loose(c, S0, got))
                flips += int((got["xc"] != c.ref(S0).xc).sum())
                total += got["xc"].size
        print(f"hp{hp}-ds{ds}: clean restatement, largest ratio {full:.3f}; with half the fp32 term {half:.3f}; "
              f"against the loose bound {lo:.3f}")
        assert full <= 1 and half <= 1
    print(f"xc: {flips} of {total} values one ulp off the reference ({flips / total:.2e})")
    assert flips / total <= 1e-3


def test_slabs_sum_exactly_and_change_nothing(cases):
    c = cases[32, 64, 17]
    base = mp.emulate(c.zx, c.P, c.S)
    for gs in (1, 2, 3, 4, 8):
        got = mp.emulate(mp.slabs(c.zx, gs), c.P, c.S)
        for k in base:
            assert np.array_equal(got[k], base[k]), (gs, k)


# mutant -> (the modes (S0) it is aimed at for a case of length S, the lengths it is aimed at)
ALL = lambda S: [S, 0]
MIXED = lambda S: [s for s in S0_MIXED if s < S]
TARGETS = {
    "taps_swapped": (ALL, lambda S: True),
    "taps_shifted": (ALL, lambda S: True),
    "no_zero_pad": (lambda S: [S], lambda S: True),
    "conv_state_off_by_one": (MIXED, lambda S: S >= 2),
    "chunk_reset": (lambda S: [S], lambda S: S >= 17),
    "no_carry": (MIXED, lambda S: S >= 2),
    "parity_wrong": (lambda S: [0] + MIXED(S), lambda S: S >= 2),
    "drop_element": (ALL, lambda S: True),
    "b_prev": (ALL, lambda S: True),
    "bc_exchanged": (ALL, lambda S: True),
    "dt_bias_neighbour": (ALL, lambda S: True),
    "a_neighbour": (ALL, lambda S: S >= 2),                # (from a zero state one step does not see dA)
    "softplus_wrong_threshold": (ALL, lambda S: True),
    "threshold_branch_clamped": (ALL, lambda S: True),
    "no_d": (ALL, lambda S: True),
    "z_neighbour": (ALL, lambda S: True),
    "slab_last_dropped": (ALL, lambda S: True),
    "y_not_rounded": (ALL, lambda S: True),
}


@pytest.mark.parametrize("mutant", mp.MUTANTS)
def test_mutant_exceeds_the_bound(cases, mutant):
    modes_of, aimed = TARGETS[mutant]
    smallest, lo, n = np.inf, np.inf, 0
    for (hp, ds, S), c in cases.items():
        if not aimed(S):
            continue
        arg = mp.drop_target(c)[0] if mutant == "drop_element" else None
        zx = mp.slabs(c.zx, 3) if mutant == "slab_last_dropped" else c.zx
        for S0 in modes_of(S):
            got = mp.emulate(zx, c.P, S0, mutant=mutant, arg=arg)
            r = worst(c, S0, got)
            assert r > 1, (c.name, S0, r)
            smallest, lo, n = min(smallest, r), min(lo, loose(c, S0, got)), n + 1
    print(f"{mutant}: smallest ratio {smallest:.3g} over {n} runs aimed at it (against the loose bound {lo:.3g})")
    assert n >= 6 and smallest > 1


def test_dropped_element_shows_in_its_named_entry(cases):
    """The probe row's one-hot B and C: the dropped update is an O(1) error of yz[row][t][p] itself."""
    for c in cases.values():
        arg, (r, t, p) = mp.drop_target(c)
        ref = c.ref(c.S)
        got = mp.emulate(c.zx, c.P, c.S, mutant="drop_element", arg=arg)
        d = abs(got["yz"][r, t, p] - ref.yz[r, t, p])
        assert d > 0.25 * abs(ref.yz[r, t, p]) > 0 and d > 100 * ref.e_yz[r, t, p], (c.name, d, ref.yz[r, t, p])


def test_iid_one_step_data_do_not_catch_a_dropped_element():
    """The data and the assertions of test_mamba_step_kernel_vs_oracle (tiny geometry: one step, i.i.d. inputs
    and states, compared after out_proj with err.max() < 0.05 * max|ref| and on the state with 2^-7 * the
    global maximum and < 1 % differing elements): the restatement with the update of one state element left
    out passes them all, which is why the probe rows exist: D = 1 on every head, so the skip term dominates y,
    and the state threshold is relative to the global maximum (for 3 in 10 of these state elements the
    whole update is below half of it; the element left out here is the one of them whose update is largest in ulps).
    The derived bound sees the same fault on the same data: that state element is off by more than its
    bound."""
    import torch
    import torch.nn.functional as F

    from oracle import hybrid_ref as HR
    c = HR.HybridCfg(d_model=256, n_layer=4, attn_layer_idx=(2,), n_heads=2, n_kv=1, d_ff=512, d_state=64, headdim=32)
    g = torch.Generator().manual_seed(0)
    W = HR.make_weights(c, seed=1)
    p = "backbone.layers.0.mixer."
    R = 6
    u = torch.randn(R, 1, c.d_model, generator=g).to(torch.bfloat16)
    cache = HR.HybridCache(c, R, 16)
    cache.conv[0] = torch.randn(R, c.conv_dim, 4, generator=g).to(torch.bfloat16)
    cache.ssm[0] = (0.5 * torch.randn(R, c.nheads_ssm, c.headdim, c.d_state, generator=g)).to(torch.bfloat16)
    conv0, ssm0 = cache.conv[0].float().numpy(), cache.ssm[0].float().numpy()
    zx = F.linear(u, W[p + "in_proj.weight"]).float().numpy()                       # [R][1][ncol]
    ref_out = HR.mamba2(W, c, 0, u, cache)
    P = mp.Params(conv_w=W[p + "conv1d.weight"].float().reshape(c.conv_dim, 4).numpy(),
                  conv_b=W[p + "conv1d.bias"].float().numpy(), A=(-torch.exp(W[p + "A_log"].float())).numpy(),
                  dt_bias=W[p + "dt_bias"].float().numpy(), D=W[p + "D"].float().numpy(),
                  norm_w=W[p + "norm.weight"].float().numpy())
    ref = mp.reference(zx, P, conv0=conv0, ssm0=ssm0, round_at=mp.round_points(1, 0))
    upd = np.abs(ref.ssm - ssm0)                                    # what a dropped update leaves out
    unseen = upd <= 0.5 * 2 ** -7 * np.abs(ref.ssm).max()
    print(f"i.i.d. one step: {unseen.mean() * 100:.0f} % of the state elements have an update below half the old "
          f"state threshold")
    assert unseen.mean() > 0.25
    elem = np.unravel_index(np.argmax(np.where(unseen, upd / mp.ulp(ref.ssm + (ref.ssm == 0)), 0.0)), upd.shape)
    passed = {}
    for mutant in (None, "drop_element"):
        got = mp.emulate(zx, P, 0, conv0=conv0, ssm0=ssm0, mutant=mutant, arg=tuple(int(i) for i in elem) + (0,))
        d = (torch.from_numpy(got["ssm"]).float() - cache.ssm[0].float()).abs()
        old_state = bool(d.max() <= 2 ** -7 * cache.ssm[0].float().abs().max() and (d > 0).float().mean() < 0.01)
        out = F.linear(torch.from_numpy(got["out"][:, 0]).to(torch.bfloat16), W[p + "out_proj.weight"])
        err = (out.float() - ref_out[:, 0].float()).abs()
        old_out = bool(err.max() < 0.05 * ref_out.float().abs().max() and err.mean() < 5e-3)
        new = max(mp.ratio(got["ssm"], ref.ssm, ref.e_ssm), mp.ratio(got["yz"], ref.yz, ref.e_yz))
        print(f"i.i.d. one step, {mutant or 'clean'}: old state assertion {'passes' if old_state else 'fails'}, "
              f"old output assertion {'passes' if old_out else 'fails'}, derived-bound ratio {new:.3g}")
        passed[mutant] = (old_state and old_out, new)
    assert passed[None][0] and passed[None][1] <= 1
    assert passed["drop_element"][0], "today's assertions were expected to miss the dropped element"
    assert passed["drop_element"][1] > 1
