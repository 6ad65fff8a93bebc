"""CPU: the attention probe helper (tests/attn_probe.py) -- the fp32 emulation of the kernels' arithmetic
stays within the derived bound, and every masking / partition error the GPU tests are there to catch
exceeds it by at least 10x. The mutations are sets of visible keys handed to the emulation: no kernel is
broken to show what the tests can see."""
import pytest
import torch

from . import attn_probe as ap
from .attn_probe import PREFILL_S, prefill_future

R, H, HK = 2, 16, 4
BLOCK_SPLITS = (1, 2, 3, 8, 24)
SLICE_SPLITS = (2, 4, 8, 16)
CTXS = [1, 33, 129, 300, 1000, 2999]
MUT = 10.0                      # a mutation must exceed the bound by this factor


def _smax(ctx):
    return (ctx // 256 + 1) * 256           # always a poisoned tail


_cache = {}


def _probes(ctx):
    """Every round's probe of ctx (all edges of both partition rules visited), built once."""
    if ctx not in _cache:
        edges = ap.edge_keys(ctx, BLOCK_SPLITS, SLICE_SPLITS)
        _cache[ctx] = [ap.decode_probe(R, H, HK, ctx, _smax(ctx), edges, seed=ctx, rnd=i)
                       for i in range(ap.n_rounds(edges, R, H, HK))]
    return _cache[ctx]


def _worst(ctx, keys):
    """Largest |out - ref| / bound over the rounds when exactly `keys` are visible."""
    return max(pr.ratio(pr.emulate(pr.visible(keys))) for pr in _probes(ctx))


def test_partitions_cover_every_key_once():
    for ctx in CTXS + [128, 256, 257]:
        for ns in BLOCK_SPLITS:
            got = sorted(j for sp in range(ns) for j in ap.block_split_keys(ctx, ns, sp))
            assert got == list(range(ctx))
        for ns in SLICE_SPLITS:
            got = sorted(j for sp in range(ns) for j in ap.slice_split_keys(ctx, ns, sp))
            assert got == list(range(ctx))
            assert ap.slice_split_keys(ctx, ns, 0) == sorted(
                j for w in range(4) for j in ap.slice_split_keys(ctx, ns, 0, wave=w))


def test_edges_are_hot_in_some_round():
    for ctx in CTXS:
        edges = ap.edge_keys(ctx, BLOCK_SPLITS, SLICE_SPLITS)
        assert all(0 <= j < ctx for j in edges) and {0, ctx - 1, ctx // 2} <= set(edges)
        hot = set(torch.cat([pr.hot.reshape(-1) for pr in _probes(ctx)]).tolist()) - {-1}
        assert hot == set(edges)
        for pr in _probes(ctx):                     # the hot cache rows are the heads' q, bit for bit
            for r, h in (pr.hot >= 0).nonzero().tolist():
                assert torch.equal(pr.k[r, h // (H // HK), pr.hot[r, h]], pr.q[r, h])


@pytest.mark.parametrize("ctx", CTXS)
def test_emulation_within_bound(ctx):
    for pr in _probes(ctx):
        ra = pr.ratio(pr.emulate())
        print(f"ctx {ctx}: emulation / bound = {ra:.3f}")
        assert ra <= 1.0
        assert float(pr.p[..., ctx:].max()) == 0.0        # the reference itself sees no poisoned key


@pytest.mark.parametrize("ctx", [c for c in CTXS if c > 1])
def test_dropped_last_key_fails(ctx):
    assert _worst(ctx, range(ctx - 1)) >= MUT


@pytest.mark.parametrize("ctx", CTXS)
def test_mask_le_reads_one_poisoned_key_fails(ctx):
    assert _worst(ctx, range(ctx + 1)) >= MUT


@pytest.mark.parametrize("ctx", CTXS)
def test_dropped_split_fails(ctx):
    for rule, splits in ((ap.block_split_keys, BLOCK_SPLITS), (ap.slice_split_keys, SLICE_SPLITS)):
        for ns in splits:
            for sp in range(ns):
                gone = set(rule(ctx, ns, sp))
                if not gone or len(gone) == ctx:
                    continue                               # an empty split; the only split
                ra = _worst(ctx, sorted(set(range(ctx)) - gone))
                assert ra >= MUT, (rule.__name__, ns, sp, ra)


@pytest.mark.parametrize("ctx", [c for c in CTXS if c > 32])
def test_dropped_wave_slice_fails(ctx):
    """Each wave's last 32-key slice (an error in the per-wave block count kbw); at ctx 1000 wave 3's is the
    last slice of the last 128-block."""
    for w in range(4):
        if ctx - 32 * w <= 0:
            continue
        b = (ctx - 32 * w + ap.AT_KB - 1) // ap.AT_KB - 1
        gone = set(ap.wave_slice_keys(ctx, b, w))
        assert gone
        ra = _worst(ctx, sorted(set(range(ctx)) - gone))
        assert ra >= MUT, (w, b, ra)
    assert list(ap.wave_slice_keys(1000, 7, 3)) == list(range(992, 1000))


def test_fp8_probe_keeps_its_preconditions():
    """decode_probe(fp8=True) re-asserts p(j*) >= 0.5 and the poison margin on the dequantised cache; the
    emulation on those values stays within the unchanged bound, a dropped last key does not."""
    from zonos_amd import kvlayout as kl
    ctx = 300
    edges = ap.edge_keys(ctx, BLOCK_SPLITS)
    pr = ap.decode_probe(R, H, HK, ctx, 512, edges, seed=5, fp8=True)
    assert torch.equal(kl.dequantize_kv_e4m3(pr.quant["kq"], pr.quant["ks"]), pr.k)
    assert pr.ratio(pr.emulate()) <= 1.0
    worst = max(p_.ratio(p_.emulate(p_.visible(range(ctx - 1))))
                for p_ in (ap.decode_probe(R, H, HK, ctx, 512, edges, seed=5, rnd=i, fp8=True)
                           for i in range(ap.n_rounds(edges, R, H, HK))))
    assert worst >= MUT


def test_newest_key_probe():
    """The fused entries' form: key ctx - 1 comes from the kernel, the input cache holds poison there."""
    ctx, smax = 129, 256
    g = torch.Generator().manual_seed(1)
    q = ap.draw_q(R, H, HK, g)
    knew = q[:, ::H // HK].clone()
    vnew = torch.randn(R, HK, ap.HD, generator=g).to(torch.bfloat16)
    pr = ap.decode_probe(R, H, HK, ctx, smax, ap.edge_keys(ctx, (1, 2)), seed=2, q=q, newest=(knew, vnew))
    assert bool((pr.hot[:, ::H // HK] == ctx - 1).all()) and int(pr.hot[:, 1].max()) < ctx - 1
    assert torch.equal(pr.k[:, :, ctx - 1], knew) and torch.equal(pr.v_in[:, :, ctx - 1], pr.v_in[:, :, ctx])
    assert torch.equal(pr.k[:, :, :ctx - 1], pr.k_in[:, :, :ctx - 1]) and torch.equal(pr.k[:, :, ctx:], pr.k_in[:, :, ctx:])
    assert pr.ratio(pr.emulate()) <= 1.0
    # the unpatched cache (poison at ctx - 1) and a dropped newest key both fail
    stale = ap.emulate(pr._qb(), pr._bh(pr.k_in), pr._bh(pr.v_in), pr.visible())
    assert pr.ratio(stale) >= MUT
    assert pr.ratio(pr.emulate(pr.visible(range(ctx - 1)))) >= MUT


@pytest.mark.parametrize("S", PREFILL_S)
def test_prefill_emulation_within_bound_and_mask_off_by_one_fails(S):
    smax = (S + 31) // 32 * 32 + 32
    for fut in ((), prefill_future(S)):
        pp = ap.prefill_probe(R, S, H, HK, smax, seed=S, future=fut)
        ra = pp.ratio(pp.emulate())
        print(f"S {S} future {list(fut)}: emulation / bound = {ra:.3f}")
        assert ra <= 1.0
        assert pp.ratio(pp.emulate(shift=1)) >= MUT        # key <= qt + 1
        # per query: the future-hot keys ruin exactly the queries t' (and the poison the last one)
        bad = ((pp.emulate(shift=1).double() - pp.ref).abs() / pp.bound).amax(dim=(0, 2, 3)) >= MUT
        assert all(bool(bad[t]) for t in list(fut) + [S - 1])
        if S > 1:
            assert pp.ratio(pp.emulate(shift=-1)) >= MUT   # key < qt: the diagonal lost
