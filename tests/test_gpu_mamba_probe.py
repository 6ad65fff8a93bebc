"""The Mamba2 mixer kernels (zonos_amd/csrc/mamba.hip) against the fp64 reference and the derived elementwise
bound of tests/mamba_probe.py, on its probe cases: zk_mamba_prefill (conv + scan), chains of zk_mamba_step /
zk_mamba_step_per_head (in place and ping-pong, every slab count), prefill followed by steps, zk_gated_rmsnorm on
both of its paths, and the step word. tests/test_mamba_probe_cpu.py shows what these cases detect. Every test
prints its figures (pytest -s); profiles/mamba_probe_tests.txt records them."""
import numpy as np
import pytest
import torch

from . import mamba_probe as mp

pytestmark = pytest.mark.gpu
DEV = "cuda"
SLACK = 4096               # elements on each side of a buffer that must stay untouched
SENTINEL = 1234.5
GEOM_IDS = [f"hp{hp}-ds{ds}" for hp, ds in mp.GEOMS]
TERMS = (1.0, 2.0, mp.F32_TERM / 1.5, mp.F32_TERM)      # the fp32 terms a result is measured with
# xc values one ulp off the reference: the fp32 restatement has 2.3e-5 of them (test_mamba_probe_cpu.py); the cap
# leaves the device's expf a margin of 40 x over that (and two values where a case has fewer than 2000)
XC_FLIP_CAP = 1e-3


@pytest.fixture(scope="module")
def cases():
    from zonos_amd import _lib
    _lib.load()
    return mp.cases()


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV).contiguous()


def _np(t):
    return t.detach().float().cpu().double().numpy()


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _sentinel(shape, dtype, fill=SENTINEL):
    """(the whole tensor, the view of `shape` in its middle), everything filled with `fill`."""
    n = int(np.prod(shape))
    big = torch.full((n + 2 * SLACK,), fill, dtype=dtype, device=DEV)
    return big, big[SLACK:SLACK + n].view(shape)


def _slack_untouched(big, fill=SENTINEL):
    ref = torch.full((SLACK,), fill, dtype=big.dtype, device=DEV)
    return torch.equal(_bits(big[:SLACK]), _bits(ref)) and torch.equal(_bits(big[-SLACK:]), _bits(ref))


def _params(c):
    P = c.P
    return dict(cw=_t(P.conv_w), cb=_t(P.conv_b), A=_t(P.A), dtb=_t(P.dt_bias), D=_t(P.D), nw=_t(P.norm_w))


def _needed_term(check):
    """The smallest of TERMS with which check(term) <= 1 (inf: none)."""
    for term in TERMS:
        if check(term) <= 1:
            return term
    return np.inf


def _prefill(c, d, S, conv, ssm, yz, xc=None):
    """zk_mamba_prefill over the first S steps of the case."""
    from zonos_amd._lib import call, ptr, stream_ptr
    zx = _t(c.zx[:, :S])
    xc = torch.zeros(mp.ROWS, S, c.conv_dim, dtype=torch.bfloat16, device=DEV) if xc is None else xc
    call("zk_mamba_prefill", ptr(zx), mp.ROWS, S, c.di, mp.NH, c.hp, c.ds, ptr(d["cw"]), ptr(d["cb"]), ptr(xc),
         ptr(conv), ptr(ssm), ptr(d["A"]), ptr(d["dtb"]), ptr(d["D"]), ptr(yz), stream_ptr())
    torch.cuda.synchronize()
    return xc


def _norm(d, yz, rows, di):
    from zonos_amd._lib import call, ptr, stream_ptr
    out = torch.zeros(rows, di, dtype=torch.bfloat16, device=DEV)
    call("zk_gated_rmsnorm", ptr(yz), rows, di, ptr(d["nw"]), mp.NORM_EPS, ptr(out), None, stream_ptr())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("S", mp.LENGTHS)
@pytest.mark.parametrize("geom", mp.GEOMS, ids=GEOM_IDS)
def test_prefill_vs_reference(cases, geom, S):
    """xc within its bound (one bf16 ulp where a flip is possible) and seldom off at all; the conv state bit
    for bit; the final SSM state, yz of every step and the norm output within the bound of the reference
    recurrence fed with the device's own xc (no flip allowance for x, B, C)."""
    c = cases[geom + (S,)]
    d = _params(c)
    R, di = mp.ROWS, c.di
    bc, conv = _sentinel((R, c.conv_dim, 4), torch.bfloat16)
    bs, ssm = _sentinel((R, mp.NH, c.hp, c.ds), torch.bfloat16)
    by, yz = _sentinel((R, S, di), torch.float32)
    xc = _np(_prefill(c, d, S, conv, ssm, yz))
    out = _np(_norm(d, yz, R * S, di)).reshape(R, S, di)
    assert _slack_untouched(bc) and _slack_untouched(bs) and _slack_untouched(by)
    ref = c.ref(S)
    r_xc = mp.ratio(xc, ref.xc, ref.e_xc)
    flips = float((xc != ref.xc).mean())
    assert np.array_equal(_np(conv), ref.conv[:, S - 1]), "conv state"
    got = dict(ssm=_np(ssm), yz=_np(yz), out=out)

    def check(term):
        own = mp.reference(c.zx, c.P, round_at=mp.round_points(S, S), xc=xc, f32_term=term)
        return max(mp.ratio(got[k], getattr(own, k), getattr(own, "e_" + k)) for k in got)
    own = mp.reference(c.zx, c.P, round_at=mp.round_points(S, S), xc=xc)
    r = {k: mp.ratio(got[k], getattr(own, k), getattr(own, "e_" + k)) for k in got}
    print(f"prefill {c.name}: xc ratio {r_xc:.3f}, xc flips {flips:.2e}, ssm {r['ssm']:.3f}, yz {r['yz']:.3f}, "
          f"norm {r['out']:.3f}, fp32 term needed {_needed_term(check):.3g} of {mp.F32_TERM}")
    assert r_xc <= 1 and flips * xc.size <= max(XC_FLIP_CAP * xc.size, 2)
    assert r["ssm"] <= 1 and r["yz"] <= 1 and r["out"] <= 1, r


def _chain(c, d, S0, S, fn, pingpong, gs, conv, ssm, yz_steps):
    """The steps S0 .. S-1 through `fn` (position t reads the parity-(t & 1) buffers). After every step the
    written conv buffer is the reference's bit for bit and the buffers that were read are unmodified."""
    from zonos_amd._lib import call, ptr, stream_ptr
    ref = c.ref(S0)
    parts = _t(mp.slabs(c.zx, gs).transpose(2, 0, 1, 3))               # [S][gs][R][ncol]
    pos = torch.zeros(1, dtype=torch.int32, device=DEV)
    s = stream_ptr()
    for t in range(S0, S):
        pos.fill_(t)
        rd = t & 1
        conv_read = conv[rd].clone()
        ssm_read = ssm[rd].clone() if pingpong else None
        call(fn, ptr(parts[t]), gs, mp.ROWS, c.di, mp.NH, c.hp, c.ds, ptr(d["cw"]), ptr(d["cb"]), ptr(conv[0]),
             ptr(conv[1]), ptr(pos), ptr(ssm[0]), ptr(ssm[1]) if pingpong else None, ptr(d["A"]), ptr(d["dtb"]),
             ptr(d["D"]), ptr(yz_steps[t - S0]), None, s)
        torch.cuda.synchronize()
        assert np.array_equal(_np(conv[rd ^ 1]), ref.conv[:, t]), f"conv state after step {t}"
        assert torch.equal(_bits(conv[rd]), _bits(conv_read)), f"conv buffer read by step {t} modified"
        if pingpong:
            assert torch.equal(_bits(ssm[rd]), _bits(ssm_read)), f"SSM buffer read by step {t} modified"
    return ssm[S & 1] if pingpong else ssm[0]


def _chain_from_zero(c, fn, pingpong, gs):
    d = _params(c)
    R, S = mp.ROWS, c.S
    conv = [torch.zeros(R, c.conv_dim, 4, dtype=torch.bfloat16, device=DEV) for _ in range(2)]
    ssm = [torch.zeros(R, mp.NH, c.hp, c.ds, dtype=torch.bfloat16, device=DEV) for _ in range(2)]
    yz = torch.zeros(S, R, c.di, device=DEV)
    last = _chain(c, d, 0, S, fn, pingpong, gs, conv, ssm, yz)
    got = dict(ssm=_np(last), yz=_np(yz).transpose(1, 0, 2))

    def check(term):
        ref = c.ref(0, term)
        return max(mp.ratio(got[k], getattr(ref, k), getattr(ref, "e_" + k)) for k in got)
    ref = c.ref(0)
    r = {k: mp.ratio(got[k], getattr(ref, k), getattr(ref, "e_" + k)) for k in got}
    print(f"steps {c.name} {fn} {'ping-pong' if pingpong else 'in place'} gs {gs}: ssm {r['ssm']:.3f}, "
          f"yz {r['yz']:.3f}, fp32 term needed {_needed_term(check):.3g} of {mp.F32_TERM}")
    assert r["ssm"] <= 1 and r["yz"] <= 1, r


@pytest.mark.parametrize("gs", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("pingpong", [False, True], ids=["inplace", "pingpong"])
@pytest.mark.parametrize("fn", ["zk_mamba_step", "zk_mamba_step_per_head"])
@pytest.mark.parametrize("geom", mp.GEOMS, ids=GEOM_IDS)
def test_step_chain_vs_reference(cases, geom, fn, pingpong, gs):
    """33 consecutive launches from zero states, pos_dev advancing: yz of every step and the final state
    within the bound (the state is stored as bf16 after every step), slabs whose fp32 sum is exact."""
    _chain_from_zero(cases[geom + (33,)], fn, pingpong, gs)


@pytest.mark.parametrize("geom", mp.GEOMS, ids=GEOM_IDS)
def test_step_chain_every_length(cases, geom):
    """The chains of the other lengths (their own data), grouped entry, ping-pong, two slabs."""
    for S in mp.LENGTHS[:-1]:
        _chain_from_zero(cases[geom + (S,)], "zk_mamba_step", True, 2)


@pytest.mark.parametrize("S0", [1, 3, 16, 17])
@pytest.mark.parametrize("geom", mp.GEOMS, ids=GEOM_IDS)
def test_prefill_then_steps(cases, geom, S0):
    """prefill(S0) into the parity-(S0 & 1) buffers, then the steps S0 .. 32 as hybrid.py issues them: all 33
    rows of yz and the final state within the bound, the final conv state that of prefill(33) bit for bit.
    The buffers the prefill does not write hold a sentinel, so a step that reads the wrong parity shows."""
    c = cases[geom + (33,)]
    d = _params(c)
    R, S, di = mp.ROWS, c.S, c.di
    conv = [torch.full((R, c.conv_dim, 4), SENTINEL, dtype=torch.bfloat16, device=DEV) for _ in range(2)]
    ssm = [torch.full((R, mp.NH, c.hp, c.ds), SENTINEL, dtype=torch.bfloat16, device=DEV) for _ in range(2)]
    yz_p = torch.zeros(R, S0, di, device=DEV)
    yz_s = torch.zeros(S - S0, R, di, device=DEV)
    _prefill(c, d, S0, conv[S0 & 1], ssm[S0 & 1], yz_p)
    ref = c.ref(S0)
    assert np.array_equal(_np(conv[S0 & 1]), ref.conv[:, S0 - 1])
    last = _chain(c, d, S0, S, "zk_mamba_step", True, 2, conv, ssm, yz_s)
    got = dict(ssm=_np(last), yz=np.concatenate([_np(yz_p), _np(yz_s).transpose(1, 0, 2)], axis=1))

    def check(term):
        rf = c.ref(S0, term)
        return max(mp.ratio(got[k], getattr(rf, k), getattr(rf, "e_" + k)) for k in got)
    r = {k: mp.ratio(got[k], getattr(ref, k), getattr(ref, "e_" + k)) for k in got}
    print(f"prefill({S0}) + steps {c.name}: ssm {r['ssm']:.3f}, yz {r['yz']:.3f}, "
          f"fp32 term needed {_needed_term(check):.3g} of {mp.F32_TERM}")
    assert r["ssm"] <= 1 and r["yz"] <= 1, r
    conv_full = torch.zeros(R, c.conv_dim, 4, dtype=torch.bfloat16, device=DEV)
    _prefill(c, d, S, conv_full, torch.zeros_like(ssm[0]), torch.zeros(R, S, di, device=DEV))
    assert torch.equal(_bits(conv[S & 1]), _bits(conv_full)), "conv state after the chain != prefill(S)'s"


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("di", [100, 4096, 4100, 8192])
def test_gated_rmsnorm_vs_reference(cases, di, rows):
    """Both paths (registers for d_inner <= 4096, the strided loop above), a row that is no multiple of the
    workgroup, against fp64 within the bf16 bound (exact inputs: the fp32 term and one ulp where a flip is
    possible); the output sits in sentinel-filled slack that stays untouched; with the step word set the
    output comes back bit-unchanged."""
    from zonos_amd._lib import call, ptr, stream_ptr
    rng = np.random.default_rng([di, rows])
    g = (rng.standard_normal((rows, di)) * np.exp(rng.uniform(-3, 3, size=(rows, di)))).astype(np.float32)
    w = rng.uniform(-1.5, 1.5, size=di).astype(np.float32)
    gd, wd = _t(g), _t(w)
    for skip in (0, 1):
        big, out = _sentinel((rows, di), torch.bfloat16)
        word = torch.full((1,), skip, dtype=torch.int32, device=DEV)
        call("zk_gated_rmsnorm", ptr(gd), rows, di, ptr(wd), mp.NORM_EPS, ptr(out), ptr(word), stream_ptr())
        torch.cuda.synchronize()
        assert _slack_untouched(big)
        if skip:
            assert torch.equal(_bits(big), _bits(torch.full_like(big, SENTINEL)))
            continue
        got = _np(out)
        terms = {}
        for term in TERMS:
            ref, e = mp.norm_reference(g.astype(np.float64), np.zeros((rows, di)), w.astype(np.float64),
                                       f32_term=term)
            terms[term] = mp.ratio(got, ref, e)
        need = min([t for t in TERMS if terms[t] <= 1], default=np.inf)
        print(f"gated_rmsnorm d_inner {di} rows {rows}: ratio {terms[mp.F32_TERM]:.3f}, flips "
              f"{float((got != ref).mean()):.2e}, fp32 term needed {need:.3g} of {mp.F32_TERM}")
        assert terms[mp.F32_TERM] <= 1


@pytest.mark.parametrize("fn", ["zk_mamba_step", "zk_mamba_step_per_head"])
@pytest.mark.parametrize("geom", mp.GEOMS, ids=GEOM_IDS)
def test_step_word_set_changes_nothing(cases, geom, fn):
    """With the step word set both conv buffers, both SSM buffers and yz come back bit-unchanged (each holds
    recognisable values inside slack); with it clear the same call writes."""
    from zonos_amd._lib import call, ptr, stream_ptr
    c = cases[geom + (5,)]
    d = _params(c)
    R = mp.ROWS
    parts = _t(mp.slabs(c.zx, 2).transpose(2, 0, 1, 3))
    rng = np.random.default_rng(7)
    shapes = dict(conv_a=(R, c.conv_dim, 4), conv_b=(R, c.conv_dim, 4), ssm_a=(R, mp.NH, c.hp, c.ds),
                  ssm_b=(R, mp.NH, c.hp, c.ds), yz=(R, c.di))
    for skip in (1, 0):
        bufs, before = {}, {}
        for i, (k, shp) in enumerate(shapes.items()):
            big, v = _sentinel(shp, torch.float32 if k == "yz" else torch.bfloat16)
            v.copy_(_t(rng.uniform(-1, 1, size=shp)).to(v.dtype) + (i + 1))
            bufs[k], before[k] = (big, v), big.clone()
        word = torch.full((1,), skip, dtype=torch.int32, device=DEV)
        pos = torch.full((1,), 3, dtype=torch.int32, device=DEV)
        call(fn, ptr(parts[3]), 2, R, c.di, mp.NH, c.hp, c.ds, ptr(d["cw"]), ptr(d["cb"]), ptr(bufs["conv_a"][1]),
             ptr(bufs["conv_b"][1]), ptr(pos), ptr(bufs["ssm_a"][1]), ptr(bufs["ssm_b"][1]), ptr(d["A"]),
             ptr(d["dtb"]), ptr(d["D"]), ptr(bufs["yz"][1]), ptr(word), stream_ptr())
        torch.cuda.synchronize()
        same = {k: torch.equal(_bits(bufs[k][0]), _bits(before[k])) for k in shapes}
        if skip:
            assert all(same.values()), same
        else:       # position 3 reads the b buffers and writes the a buffers and yz
            assert same == dict(conv_a=False, conv_b=True, ssm_a=False, ssm_b=True, yz=False), same
            assert all(_slack_untouched(big) for big, _ in bufs.values())
