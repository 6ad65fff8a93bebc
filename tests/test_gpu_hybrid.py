"""Hybrid (Mamba2 + attention) backbone on the GPU vs the CPU restatement of mamba_ssm's
semantics (oracle/hybrid_ref.py). mamba_ssm / causal-conv1d / flash-attn and the hybrid
checkpoint are absent here, so parity with the reference hybrid itself is UNPINNED; these
tests pin the HIP engine to the restatement (kernels and whole generate())."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import hybrid_ref as HR
from oracle import zonos_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"

TINYH = HR.HybridCfg(d_model=256, n_layer=4, attn_layer_idx=(2,), n_heads=2, n_kv=1, d_ff=512, d_state=64,
                     headdim=32)


def _engine(W, c=TINYH):
    from zonos_amd.hybrid import HybridDecoder, HybridEngineConfig
    ec = HybridEngineConfig(d_model=c.d_model, n_layer=c.n_layer, attn_layer_idx=c.attn_layer_idx, n_heads=c.n_heads,
                            n_kv=c.n_kv, d_ff=c.d_ff, d_state=c.d_state, headdim=c.headdim, eps=c.eps, d_mlp=c.d_mlp,
                            rms_norm=c.rms_norm, residual_in_fp32=c.residual_in_fp32)
    return HybridDecoder(ec, W, DEV)


# The BackboneConfig variants the reference's mamba_ssm backbone honours (_mamba_ssm.py:18-31,49-57):
# rms_norm, residual_in_fp32, an MLP on the Mamba2 blocks (d_intermediate != 0), and all three.
# Parity with mamba_ssm unpinned (absent); pinned to the restatement's published semantics.
VARIANTS = {
    "rms": dict(rms_norm=True),
    "fp32res": dict(residual_in_fp32=True),
    "mamba_mlp": dict(d_mlp=384),
    "all": dict(rms_norm=True, residual_in_fp32=True, d_mlp=256),
}


def _variant(name, base=None):
    import dataclasses
    return dataclasses.replace(base or TINYH, **VARIANTS[name])


# one Mamba2 layer at the full hybrid widths (D 2048, d_inner 4096, d_state 128, headdim 64, 64 heads)
FULL1 = HR.HybridCfg(n_layer=1, attn_layer_idx=())


@pytest.mark.parametrize("c", [TINYH, FULL1], ids=["tiny", "full_width"])
def test_mamba_step_kernel_vs_oracle(c):
    """zk_mamba_step (slab reduce + conv update + SSM update + gate) and zk_gated_rmsnorm on one
    decode step against the oracle's Mamba2 recurrence with the same inputs and states."""
    from zonos_amd._lib import call, ptr, stream_ptr
    g = torch.Generator().manual_seed(0)
    W = HR.make_weights(c, seed=1)
    i = 0
    p = f"backbone.layers.{i}.mixer."
    R, gs = 6, 3
    u = torch.randn(R, 1, c.d_model, generator=g).to(torch.bfloat16)
    cache = HR.HybridCache(c, R, 16)
    cache.conv[i] = torch.randn(R, c.conv_dim, 4, generator=g).to(torch.bfloat16)
    cache.ssm[i] = (0.5 * torch.randn(R, c.nheads_ssm, c.headdim, c.d_state, generator=g)).to(torch.bfloat16)
    conv0, ssm0 = cache.conv[i].clone(), cache.ssm[i].clone()
    # in_proj output as gs split-K slabs whose bf16-rounded sum equals the oracle's bf16 GEMM output
    zx = F.linear(u, W[p + "in_proj.weight"])[:, 0].float()             # [R][nin] (bf16 values)
    parts = torch.stack([zx * 0.5, zx * 0.25, zx * 0.25])                # exact in fp32
    ref_out = HR.mamba2(W, c, i, u, cache)                                # updates cache
    # HIP
    s = stream_ptr()
    cw = W[p + "conv1d.weight"].float().reshape(c.conv_dim, 4).to(DEV)
    cb = W[p + "conv1d.bias"].float().to(DEV)
    A = (-torch.exp(W[p + "A_log"].float())).to(DEV)
    dtb, Dv = W[p + "dt_bias"].float().to(DEV), W[p + "D"].float().to(DEV)
    pos = torch.tensor([7], dtype=torch.int32, device=DEV)               # odd: reads buffer b, writes a
    cs_a = torch.zeros(R, c.conv_dim, 4, dtype=torch.bfloat16, device=DEV)
    cs_b = conv0.to(DEV)
    ssm = ssm0.to(DEV)
    yz = torch.empty(R, c.d_inner, device=DEV)
    call("zk_mamba_step", ptr(parts.to(DEV).contiguous()), gs, R, c.d_inner, c.nheads_ssm, c.headdim, c.d_state,
         ptr(cw), ptr(cb), ptr(cs_a), ptr(cs_b), ptr(pos), ptr(ssm), None, ptr(A), ptr(dtb), ptr(Dv), ptr(yz), None,
         s)
    ym = torch.empty(R, c.d_inner, dtype=torch.bfloat16, device=DEV)
    nw = W[p + "norm.weight"].float().to(DEV)
    call("zk_gated_rmsnorm", ptr(yz), R, c.d_inner, ptr(nw), 1e-5, ptr(ym), None, s)
    torch.cuda.synchronize()
    assert torch.equal(cs_a.cpu(), cache.conv[i])                         # conv state: exact
    d = (ssm.cpu().float() - cache.ssm[i].float()).abs()
    assert d.max() <= 2 ** -7 * cache.ssm[i].float().abs().max() and (d > 0).float().mean() < 0.01
    out = F.linear(ym.cpu(), W[p + "out_proj.weight"])
    err = (out.float() - ref_out[:, 0].float()).abs()
    assert err.max() < 0.05 * ref_out.float().abs().max() and err.mean() < 5e-3, (err.max(), err.mean())
    # the derived elementwise bound (tests/mamba_probe.py) on the state and on yz before out_proj
    from . import mamba_probe as mp
    P = mp.Params(conv_w=cw.cpu().numpy(), conv_b=cb.cpu().numpy(), A=A.cpu().numpy(), dt_bias=dtb.cpu().numpy(),
                  D=Dv.cpu().numpy(), norm_w=nw.cpu().numpy())
    ref = mp.reference(parts.numpy()[:, :, None, :], P, conv0=conv0.float().numpy(), ssm0=ssm0.float().numpy(),
                       round_at=mp.round_points(1, 0))
    r_ssm = mp.ratio(ssm.cpu().float().numpy(), ref.ssm, ref.e_ssm)
    r_yz = mp.ratio(yz.cpu().numpy(), ref.yz[:, 0], ref.e_yz[:, 0])
    r_out = mp.ratio(ym.cpu().float().numpy(), ref.out[:, 0], ref.e_out[:, 0])
    print(f"derived bound: ssm {r_ssm:.3f}, yz {r_yz:.3f}, norm {r_out:.3f}")
    assert r_ssm <= 1 and r_yz <= 1 and r_out <= 1, (r_ssm, r_yz, r_out)


def test_hybrid_generate_teacher_forced_logits():
    """Whole generate() (prefill: causal conv + recurrence scan, NeoX-RoPE attention; decode:
    graph of mamba_step / attention / GEMMs) on the oracle's own greedy history: per-step CFG
    logits within bf16 tolerance, tokens equal where the decision margin is clear."""
    c = TINYH
    W = HR.make_weights(c, seed=2, head_scale=4.0)
    B, Lc, P, new = 3, 12, 4, 24
    cond = zonos_ref.synthetic_conditioning(B, Lc, c.d_model)
    prefix = zonos_ref.synthetic_prefix_codes(B, P)
    sp = dict(temperature=0.0, top_p=0, top_k=0, min_p=0, linear=0, conf=0, quad=0, repetition_penalty=1.0,
              repetition_penalty_window=2)
    tr = {}
    zonos_ref.generate(W, c, cond, prefix, new, 2.0, B, sp, seed=3, trace=tr)
    gold = tr["delayed"]
    eng = _engine(W)
    trace = {}
    offs = []

    def force(frame, step):
        off = P + 1 + step
        offs.append(off)
        if frame.shape[2]:
            frame.copy_(gold[..., off:off + 1].to(frame.device))
        return True

    eng.generate(cond.to(DEV), prefix.to(DEV), new, 2.0, B, sp, seed=3, trace=trace,
                 callback=lambda f, s, n: force(f, s), _after_prefill=lambda f: force(f, 0))
    n = min(len(trace["logits"]), len(tr["logits"]))
    assert n >= new // 2
    worst = 0.0
    for s in range(n):
        ref = tr["logits"][s].float().numpy()
        got = trace["logits"][s].cpu().numpy()
        fin = np.isfinite(ref)
        assert np.array_equal(fin, np.isfinite(got))
        e = np.abs(got[fin] - ref[fin])
        worst = max(worst, float(e.max()))
        assert e.max() < 0.5 and e.mean() < 0.05, (s, e.max(), e.mean())
    print("hybrid teacher-forced logits: steps", n, "max abs err", worst)


@pytest.mark.parametrize("name", list(VARIANTS))
def test_hybrid_variant_teacher_forced_logits(name):
    """the hybrid config variants run (no longer refused) and the whole generate() --
    prefill, the graph-captured C decode step, the first block's own norm launch, the fp32 residual
    stream, the Mamba-block MLP -- follows the restatement on its own greedy history: CFG logits within
    the base hybrid test's bounds, tokens equal where the decision margin is clear."""
    c = _variant(name)
    W = HR.make_weights(c, seed=2, head_scale=4.0)
    assert ("backbone.layers.0.norm.bias" in W) == (not c.rms_norm)
    assert ("backbone.layers.0.mlp.fc1.weight" in W) == bool(c.d_mlp)
    B, Lc, P, new = 3, 12, 4, 20
    cond = zonos_ref.synthetic_conditioning(B, Lc, c.d_model)
    prefix = zonos_ref.synthetic_prefix_codes(B, P)
    sp = dict(temperature=0.0, top_p=0, top_k=0, min_p=0, linear=0, conf=0, quad=0, repetition_penalty=1.0,
              repetition_penalty_window=2)
    tr = {}
    zonos_ref.generate(W, c, cond, prefix, new, 2.0, B, sp, seed=3, trace=tr)
    gold = tr["delayed"]
    eng = _engine(W, c)
    assert eng.cfg.norm_flags == (2 if c.rms_norm else 0) | (4 if c.residual_in_fp32 else 0)
    trace = {}

    def force(frame, step):
        off = P + 1 + step
        if frame.shape[2]:
            frame.copy_(gold[..., off:off + 1].to(frame.device))
        return True

    eng.generate(cond.to(DEV), prefix.to(DEV), new, 2.0, B, sp, seed=3, trace=trace,
                 callback=lambda f, s_, n: force(f, s_), _after_prefill=lambda f: force(f, 0))
    n = min(len(trace["logits"]), len(tr["logits"]))
    assert n >= new // 2
    worst, checked = 0.0, 0
    for st in range(n):
        ref = tr["logits"][st].float().numpy()
        got = trace["logits"][st].cpu().numpy()
        fin = np.isfinite(ref)
        assert np.array_equal(fin, np.isfinite(got))
        e = np.abs(got[fin] - ref[fin])
        worst = max(worst, float(e.max()))
        assert e.max() < 0.5 and e.mean() < 0.05, (name, st, e.max(), e.mean())
        r = np.where(fin, ref, -np.inf).reshape(-1, ref.shape[-1])
        g_ = np.where(fin, got, -np.inf).reshape(-1, ref.shape[-1])
        top2 = np.sort(r, axis=-1)[:, -2:]
        clear = (top2[:, 1] - top2[:, 0]) > 0.6
        checked += int(clear.sum())
        assert np.array_equal(r[clear].argmax(-1), g_[clear].argmax(-1)), (name, st)
    print(f"hybrid variant {name}: steps {n}, max |d| {worst:.3f}, clear decisions checked {checked}")
    assert checked > 0


@pytest.mark.parametrize("name", ["fp32res", "all"])
def test_c_hybrid_variant_step_equals_python_sequence(name, monkeypatch):
    """The variants through the C ABI (zk_hybrid_prefill / zk_hybrid_decode_step with norm_flags, d_mlp,
    xf) == the same sequence issued from Python, bit for bit, and the graph replay == eager."""
    from zonos_amd.hybrid import HybridDecoder
    c = _variant(name)
    W = HR.make_weights(c, seed=7, head_scale=4.0)
    eng = _engine(W, c)
    B = 3
    cond = zonos_ref.synthetic_conditioning(B, 12, c.d_model, seed=2).to(DEV)
    prefix = zonos_ref.synthetic_prefix_codes(B, 3, seed=4).to(DEV)
    sp = dict(temperature=1.0, top_p=0, top_k=0, min_p=0, linear=0.65, conf=0.4, quad=0.0, repetition_penalty=2.5,
              repetition_penalty_window=8)
    outs = []
    for flag in (True, False):
        monkeypatch.setattr(HybridDecoder, "c_step", flag)
        eng._ws = None
        trace = {}
        out = eng.generate(cond, prefix, 16, 2.0, B, sp, seed=9, trace=trace)
        outs.append(([o.cpu() for o in out], [t.cpu() for t in trace["logits"]]))
    (ca, la), (cb, lb) = outs
    assert all(torch.equal(x, y) for x, y in zip(ca, cb)) and len(ca) == len(cb)
    assert len(la) == len(lb) and all(torch.equal(x, y) for x, y in zip(la, lb))
    monkeypatch.setattr(HybridDecoder, "c_step", True)
    g = eng.generate(cond, prefix, 16, 2.0, B, sp, seed=9, poll_every=4)
    assert all(torch.equal(x.cpu(), y) for x, y in zip(g, ca))


def test_hybrid_variant_plugin_matches_oracle():
    """HipHybridBackbone built from a BackboneConfig with all three variants (RMSNorm blocks without
    bias parameters, fp32 residual, Mamba-block MLPs): state-dict names load unchanged and forward
    (prefill + decodes) follows the restatement."""
    from zonos.backbone import BACKBONES
    from zonos_amd.config import BackboneConfig, InferenceParams
    c = _variant("all")
    W = HR.make_weights(c, seed=6)
    bb = BACKBONES["mamba_ssm"](BackboneConfig(**c.to_zonos_config()["backbone"]))
    sd = {k[len("backbone."):]: v for k, v in W.items() if k.startswith("backbone.")}
    bb.load_state_dict(sd, strict=True)
    bb = bb.to(DEV, torch.bfloat16)
    R, S, n_dec = 4, 10, 4
    g = torch.Generator().manual_seed(8)
    xs = torch.randn(R, S + n_dec, c.d_model, generator=g).bfloat16()
    ip = InferenceParams(max_seqlen=S + n_dec, max_batch_size=R,
                         key_value_memory_dict=bb.allocate_inference_cache(R, S + n_dec),
                         lengths_per_sample=torch.zeros(R, dtype=torch.int32))
    cache = HR.HybridCache(c, R, S + n_dec)
    rot = HR.rotary_table(16384, c.head_dim)
    errs = []
    for step in range(n_dec + 1):
        sl = slice(0, S) if step == 0 else slice(S + step - 1, S + step)
        got = bb(xs[:, sl].to(DEV), ip).float().cpu()
        exp = HR.backbone(W, c, xs[:, sl], cache, rot).float()
        nn_ = sl.stop - sl.start
        ip.seqlen_offset += nn_
        ip.lengths_per_sample += nn_
        cache.seqlen_offset += nn_
        cache.lengths += nn_
        e = (got - exp).abs()
        errs.append((float(e.max()), float(e.mean())))
    print("hybrid variant plugin vs oracle |d| (max, mean) per call:", errs)
    assert max(e[0] for e in errs) < 0.15 and max(e[1] for e in errs) < 0.015, errs


@pytest.mark.parametrize("hp,ds,nh,R,gs,pos", [(32, 64, 16, 6, 2, 5), (64, 128, 64, 8, 2, 6), (64, 128, 64, 3, 1, 7),
                                               (64, 64, 16, 4, 4, 2)])
def test_mamba_step_grouped_equals_per_head(hp, ds, nh, R, gs, pos, monkeypatch):
    """Double-buffered SSM state (read buffer pos & 1, write the other) == in place, bit for bit, in
    both kernels. The grouped decode kernel (heads per workgroup, B/C conv once per group, pipelined state
    slices, whole-line state access at d_state 128) == the per-head kernel: SSM and conv states
    bit for bit; the gated outputs bit for bit, or -- where the row sum y = C.h is reduced in a
    different order (d_state 128: 16 lanes x 8 instead of 4 threads x 32) -- within 1 bf16 ulp of y."""
    from zonos_amd._lib import call, ptr, stream_ptr
    g = torch.Generator().manual_seed(hp + ds + R)
    di = nh * hp
    conv_dim = di + 2 * ds
    ncol = 2 * di + 2 * ds + nh
    parts = (torch.randn(gs, R, ncol, generator=g) * 0.5).to(DEV)
    cw = (torch.randn(conv_dim, 4, generator=g) * 0.3).to(DEV)
    cb = (torch.randn(conv_dim, generator=g) * 0.1).to(DEV)
    conv0 = torch.randn(R, conv_dim, 4, generator=g).to(torch.bfloat16)
    ssm0 = (0.5 * torch.randn(R, nh, hp, ds, generator=g)).to(torch.bfloat16)
    A = (-torch.rand(nh, generator=g) * 4).to(DEV)
    dtb = (torch.randn(nh, generator=g) * 0.5).to(DEV)
    Dv = torch.randn(nh, generator=g).to(DEV)
    posd = torch.tensor([pos], dtype=torch.int32, device=DEV)
    s = stream_ptr()
    outs = []
    for grouped, pingpong in (("0", False), ("1", False), ("1", True), ("0", True)):
        fn = "zk_mamba_step" if grouped == "1" else "zk_mamba_step_per_head"
        ca, cbuf = conv0.to(DEV), conv0.to(DEV)
        ssm = ssm0.to(DEV)
        yz = torch.full((R, di), float("nan"), device=DEV)
        if pingpong:       # {a, b}: the step at position pos reads (pos & 1) and writes the other
            other = torch.full_like(ssm, float("nan"))
            sa, sb = (other, ssm) if pos & 1 else (ssm, other)
            call(fn, ptr(parts), gs, R, di, nh, hp, ds, ptr(cw), ptr(cb), ptr(ca), ptr(cbuf), ptr(posd),
                 ptr(sa), ptr(sb), ptr(A), ptr(dtb), ptr(Dv), ptr(yz), None, s)
            torch.cuda.synchronize()
            assert torch.equal(ssm.cpu(), ssm0), "ping-pong read buffer modified"
            ssm = other
        else:
            call(fn, ptr(parts), gs, R, di, nh, hp, ds, ptr(cw), ptr(cb), ptr(ca), ptr(cbuf), ptr(posd),
                 ptr(ssm), None, ptr(A), ptr(dtb), ptr(Dv), ptr(yz), None, s)
            torch.cuda.synchronize()
        outs.append((ca.cpu(), cbuf.cpu(), ssm.cpu(), yz.cpu()))
    for i, j in ((1, 2), (0, 3)):       # ping-pong == in place, bit for bit, in each kernel
        for a, b in zip(outs[i], outs[j]):
            assert torch.equal(a, b)
    for a, b, name in zip(outs[0][:3], outs[1][:3], ("conv_a", "conv_b", "ssm")):
        assert torch.equal(a, b), name
    ya, yb = outs[0][3], outs[1][3]
    if ds != 128:
        assert torch.equal(ya, yb)
    else:
        d = (ya - yb).abs()
        assert float((d / ya.abs().clamp_min(1e-3)).max()) <= 2 ** -7 and float((d > 0).float().mean()) < 0.05


def test_hybrid_full_width_shallow_teacher_forced_logits():
    """Full hybrid widths at 4 layers (Mamba2, Mamba2, attention, Mamba2): the per-depth error of
    the full-geometry test below, with the same tolerances as TINYH (which has 4 layers too)."""
    c = HR.HybridCfg(n_layer=4, attn_layer_idx=(2,))
    W = HR.make_weights(c, seed=6, head_scale=4.0)
    B, Lc, P, new = 12, 16, 4, 8
    cond = zonos_ref.synthetic_conditioning(B, Lc, c.d_model)
    prefix = zonos_ref.synthetic_prefix_codes(B, P)
    sp = dict(temperature=0.0, top_p=0, top_k=0, min_p=0, linear=0, conf=0, quad=0, repetition_penalty=1.0,
              repetition_penalty_window=2)
    tr = {}
    zonos_ref.generate(W, c, cond, prefix, new, 2.0, B, sp, seed=3, trace=tr)
    gold = tr["delayed"]
    eng = _engine(W, c)
    trace = {}

    def force(frame, step):
        off = P + 1 + step
        if frame.shape[2]:
            frame.copy_(gold[..., off:off + 1].to(frame.device))
        return True

    eng.generate(cond.to(DEV), prefix.to(DEV), new, 2.0, B, sp, seed=3, trace=trace,
                 callback=lambda f, s, n: force(f, s), _after_prefill=lambda f: force(f, 0))
    n = min(len(trace["logits"]), len(tr["logits"]))
    errs = []
    for s in range(n):
        ref = tr["logits"][s].float().numpy()
        got = trace["logits"][s].cpu().numpy()
        fin = np.isfinite(ref)
        e = np.abs(got[fin] - ref[fin])
        errs.append((float(e.max()), float(e.mean()), float(np.abs(ref[fin]).mean())))
    print("hybrid full width, 4 layers: (max |d|, mean |d|, mean |logit|) per step:", errs)
    assert max(e[0] for e in errs) < 0.5 and max(e[1] for e in errs) < 0.05, errs


def test_hybrid_full_geometry_teacher_forced_logits():
    """The c5 geometry (synthetic.ZONOS_V01_HYBRID = HybridCfg defaults: 46 layers, D 2048, Mamba2
    d_state 128 / headdim 64 / 64 heads, attention at 9/18/27/36/45 with 16/4 heads, FFN 8192,
    heads 9x1026) at B = 12 (24 rows: the k_gemm_ws / mamba-step regime of the c5 benchmark),
    whole generate() teacher-forced on the oracle's greedy history: per-step CFG logits within
    bf16 tolerance. Pins the HIP engine to the restatement at full width; parity with mamba_ssm
    itself stays unpinned (no hybrid checkpoint or mamba_ssm here)."""
    c = HR.HybridCfg()
    W = HR.make_weights(c, seed=5, head_scale=4.0)
    B, Lc, P, new = 12, 16, 4, 12
    cond = zonos_ref.synthetic_conditioning(B, Lc, c.d_model)
    prefix = zonos_ref.synthetic_prefix_codes(B, P)
    sp = dict(temperature=0.0, top_p=0, top_k=0, min_p=0, linear=0, conf=0, quad=0, repetition_penalty=1.0,
              repetition_penalty_window=2)
    tr = {}
    zonos_ref.generate(W, c, cond, prefix, new, 2.0, B, sp, seed=3, trace=tr)
    gold = tr["delayed"]
    eng = _engine(W, c)
    del W
    trace = {}

    def force(frame, step):
        off = P + 1 + step
        if frame.shape[2]:
            frame.copy_(gold[..., off:off + 1].to(frame.device))
        return True

    eng.generate(cond.to(DEV), prefix.to(DEV), new, 2.0, B, sp, seed=3, trace=trace,
                 callback=lambda f, s, n: force(f, s), _after_prefill=lambda f: force(f, 0))
    n = min(len(trace["logits"]), len(tr["logits"]))
    assert n >= new
    # bf16 noise grows with depth: TINYH (4 layers, same head scale) differs by <= 0.05 mean; 46 layers
    # measured 0.19-0.20 mean / <= 1.22 max on logits of mean magnitude 4-5 (std 5-6), flat over the
    # decode steps (a decode-path bug would grow). Bounds: mean |d| <= 6 % of mean |logit|, and every
    # greedy decision whose reference top-1/top-2 margin exceeds twice the max error equal.
    errs, checked, total = [], 0, 0
    for s in range(n):
        ref = tr["logits"][s].float().numpy()
        got = trace["logits"][s].cpu().numpy()
        fin = np.isfinite(ref)
        assert np.array_equal(fin, np.isfinite(got))
        e = np.abs(got[fin] - ref[fin])
        errs.append((float(e.max()), float(e.mean()), float(np.abs(ref[fin]).mean())))
        r = np.where(fin, ref, -np.inf).reshape(-1, ref.shape[-1])
        g = np.where(fin, got, -np.inf).reshape(-1, ref.shape[-1])
        top2 = np.sort(r, axis=-1)[:, -2:]
        clear = (top2[:, 1] - top2[:, 0]) > 2.5
        total += len(r)
        checked += int(clear.sum())
        assert np.array_equal(r[clear].argmax(-1), g[clear].argmax(-1)), s
    print("hybrid full geometry teacher-forced logits (max |d|, mean |d|, mean |logit|) per step:", errs,
          f"decisions checked {checked}/{total}")
    assert max(e[1] / e[2] for e in errs) < 0.06 and max(e[0] for e in errs) < 2.0, errs
    assert checked >= 0.1 * total, (checked, total)


def test_hybrid_c5_batch64_teacher_forced_logits():
    """Config c5's batch: the full hybrid geometry at B = 64 (128 rows, the benchmark's regime), four
    utterances spread over the batch (0, 21, 42, 63) teacher-forced on the oracle's greedy history,
    the other 60 free-running beside them. Utterances are independent, so the oracle runs only the
    four (as a B = 4 batch of their cond / uncond rows); the engine's rows of those utterances must
    match it within the full-geometry bounds above. Parity with mamba_ssm itself stays unpinned."""
    c = HR.HybridCfg()
    W = HR.make_weights(c, seed=5, head_scale=4.0)
    B, Lc, P, new = 64, 16, 4, 3
    subset = [0, 21, 42, 63]
    cond = zonos_ref.synthetic_conditioning(B, Lc, c.d_model, seed=11)
    prefix = zonos_ref.synthetic_prefix_codes(B, P, seed=12)
    sp = dict(temperature=0.0, top_p=0, top_k=0, min_p=0, linear=0, conf=0, quad=0, repetition_penalty=1.0,
              repetition_penalty_window=2)
    idx = torch.tensor(subset)
    cond_s = torch.cat([cond[idx], cond[B + idx]])
    tr = {}
    zonos_ref.generate(W, c, cond_s, prefix[idx], new, 2.0, len(subset), sp, seed=3, trace=tr)
    gold = tr["delayed"]
    eng = _engine(W, c)
    del W
    trace = {}
    didx = idx.to(DEV)

    def force(frame, step):
        off = P + 1 + step
        if frame.shape[2]:
            frame[didx] = gold[..., off:off + 1].to(frame.device)
        return True

    eng.generate(cond.to(DEV), prefix.to(DEV), new, 2.0, B, sp, seed=3, trace=trace,
                 callback=lambda f, s, n: force(f, s), _after_prefill=lambda f: force(f, 0))
    n = min(len(trace["logits"]), len(tr["logits"]))
    assert n >= new
    errs = []
    for s in range(n):
        ref = tr["logits"][s].float().numpy()
        got = trace["logits"][s][didx].cpu().numpy()
        fin = np.isfinite(ref)
        assert np.array_equal(fin, np.isfinite(got))
        e = np.abs(got[fin] - ref[fin])
        errs.append((float(e.max()), float(e.mean()), float(np.abs(ref[fin]).mean())))
        r = np.where(fin, ref, -np.inf).reshape(-1, ref.shape[-1])
        g = np.where(fin, got, -np.inf).reshape(-1, ref.shape[-1])
        top2 = np.sort(r, axis=-1)[:, -2:]
        clear = (top2[:, 1] - top2[:, 0]) > 2.5
        assert np.array_equal(r[clear].argmax(-1), g[clear].argmax(-1)), s
    print("hybrid c5 B=64 teacher-forced logits (max |d|, mean |d|, mean |logit|) per step:", errs)
    assert max(e[1] / e[2] for e in errs) < 0.06 and max(e[0] for e in errs) < 2.0, errs


@pytest.mark.parametrize("geom,B", [("tiny", 3), ("full4", 12)])
def test_c_hybrid_step_equals_python_sequence(geom, B, monkeypatch):
    """zk_hybrid_prefill + zk_hybrid_decode_step (the hybrid prefill and decode step enqueued by the
    C ABI, so a non-Python host can drive config c5) == the same launch sequences issued from
    Python (HybridDecoder with c_step off): identical per-step logits and codes, eager; and the
    hipGraph replay of the C step gives the eager codes."""
    from zonos_amd.hybrid import HybridDecoder
    c = TINYH if geom == "tiny" else HR.HybridCfg(n_layer=4, attn_layer_idx=(2,))
    W = HR.make_weights(c, seed=7, head_scale=4.0)
    eng = _engine(W, c)
    cond = zonos_ref.synthetic_conditioning(B, 12, c.d_model, seed=2).to(DEV)
    prefix = zonos_ref.synthetic_prefix_codes(B, 3, seed=4).to(DEV)
    sp = dict(temperature=1.0, top_p=0, top_k=0, min_p=0, linear=0.65, conf=0.4, quad=0.0, repetition_penalty=2.5,
              repetition_penalty_window=8)
    outs = []
    for flag in (True, False):
        monkeypatch.setattr(HybridDecoder, "c_step", flag)
        eng._ws = None
        trace = {}
        out = eng.generate(cond, prefix, 16, 2.0, B, sp, seed=9, trace=trace)
        outs.append(([o.cpu() for o in out], [t.cpu() for t in trace["logits"]]))
    (ca, la), (cb, lb) = outs
    assert all(torch.equal(x, y) for x, y in zip(ca, cb)) and len(ca) == len(cb)
    assert len(la) == len(lb) and all(torch.equal(x, y) for x, y in zip(la, lb))
    monkeypatch.setattr(HybridDecoder, "c_step", True)
    g = eng.generate(cond, prefix, 16, 2.0, B, sp, seed=9, poll_every=4)          # hipGraph of the C step
    assert all(torch.equal(x.cpu(), y) for x, y in zip(g, ca))


def test_hybrid_backbone_plugin_matches_oracle():
    """BACKBONES["mamba_ssm"] / ["hip_hybrid"] (HipHybridBackbone, the reference's
    MambaSSMZonosBackbone plugin on the HIP kernels) through the plugin interface
    (_mamba_ssm.py:38-57): allocate_inference_cache + forward(prefill of 12 positions) + 6
    single-token decodes, vs the restatement's backbone on the same inputs (parity with mamba_ssm
    itself unpinned)."""
    from zonos.backbone import BACKBONES
    from zonos_amd.config import BackboneConfig, InferenceParams
    c = TINYH
    assert BACKBONES["mamba_ssm"] is BACKBONES["hip_hybrid"]
    assert "hybrid" in BACKBONES["mamba_ssm"].supported_architectures
    W = HR.make_weights(c, seed=6)
    bb = BACKBONES["mamba_ssm"](BackboneConfig(**c.to_zonos_config()["backbone"]))
    bb.load_state_dict({k[len("backbone."):]: v for k, v in W.items() if k.startswith("backbone.")})
    bb = bb.to(DEV, torch.bfloat16)
    R, S, n_dec = 4, 12, 6
    g = torch.Generator().manual_seed(8)
    xs = torch.randn(R, S + n_dec, c.d_model, generator=g).bfloat16()
    ip = InferenceParams(max_seqlen=S + n_dec, max_batch_size=R,
                         key_value_memory_dict=bb.allocate_inference_cache(R, S + n_dec),
                         lengths_per_sample=torch.zeros(R, dtype=torch.int32))
    cache = HR.HybridCache(c, R, S + n_dec)
    rot = HR.rotary_table(16384, c.head_dim)
    errs = []
    for step in range(n_dec + 1):
        sl = slice(0, S) if step == 0 else slice(S + step - 1, S + step)
        got = bb(xs[:, sl].to(DEV), ip).float().cpu()
        exp = HR.backbone(W, c, xs[:, sl], cache, rot).float()
        n = sl.stop - sl.start
        ip.seqlen_offset += n
        ip.lengths_per_sample += n
        cache.seqlen_offset += n
        cache.lengths += n
        e = (got - exp).abs()
        errs.append((float(e.max()), float(e.mean())))
    print("hybrid plugin vs oracle |d| (max, mean) per call:", errs)
    # LayerNorm'd outputs (|x| ~ 1): bf16 ulps plus the SSM state's bf16 rounding
    assert max(e[0] for e in errs) < 0.15 and max(e[1] for e in errs) < 0.015, errs
    # the Mamba states the plugin advanced equal the restatement's within bf16 rounding: the conv
    # state holds in_proj outputs (bf16), whose GEMM reduction order differs from the CPU's
    for i in (0, 1, 3):
        conv, ssm = ip.key_value_memory_dict[i]
        par = (S + n_dec) & 1                                # parity buffer the next step reads
        dc = (conv[par].float().cpu() - cache.conv[i].float()).abs()
        # (the in_proj input differs by the upstream layers' bf16 ulps as well: measured max 0.016)
        assert dc.max() <= 0.05 and dc.mean() <= 2e-3, (float(dc.max()), float(dc.mean()))
        d = (ssm[par].float().cpu() - cache.ssm[i].float()).abs()
        assert d.max() <= 2 ** -6 * cache.ssm[i].float().abs().max(), float(d.max())


# c5 long-run bounds from the measured error growth on MI355X (profiles/r4_hybrid_c5_long_test.txt):
# fp32 CFG logits of the engine (decode-step graph at B = 64, 2570 teacher-forced steps) vs the
# restatement, max 0.22-0.28 / mean 0.043-0.046 at every recorded step from 0 to 2570 -- flat, no drift
# of the recurrent bf16 SSM states. Bounds = 1.4x the measured worst step; the late steps' mean error
# may not exceed the first steps' by more than 25 %.
C5_MAX, C5_MEAN, C5_DRIFT = 0.4, 0.065, 1.25


def test_hybrid_c5_workload_teacher_forced_long():
    """The hybrid where the c5 benchmark runs it: full hybrid geometry (46 layers, Mamba2 d_state 128,
    attention at 9/18/27/36/45), B = 64 (R = 128: the k_gemm_ws regime), Lc = 400, P = 10, teacher-forced
    for 2570 steps on a seeded history -- the bf16 SSM states after thousands of recurrent updates and
    NeoX-RoPE attention at contexts up to 2980 -- vs the restatement's own teacher-forced run
    (tests/golden/gen_hybrid_c5.npz, three utterances of the batch; parity with mamba_ssm unpinned)."""
    import os

    from zonos_amd.hybrid import HybridDecoder, HybridEngineConfig

    from .golden_util import CLI_SP, G, HYBRID_C5, forced_history, wsum
    c, cfg = HYBRID_C5, HR.ZONOS_V01_HYBRID
    d = np.load(os.path.join(G, "gen_hybrid_c5.npz"))
    W = HR.make_weights(cfg, seed=c["w_seed"])
    assert wsum(W) == str(d["wsum"])
    B, Lc, P, T = c["B"], c["Lc"], c["P"], c["T"]
    cond = zonos_ref.synthetic_conditioning(B, Lc, cfg.d_model, seed=c["cond_seed"])
    prefix = zonos_ref.synthetic_prefix_codes(B, P, seed=c["prefix_seed"])
    hist = forced_history(B, P, T, prefix, seed=c["hist_seed"]).to(DEV)
    ec = HybridEngineConfig(d_model=cfg.d_model, n_layer=cfg.n_layer, attn_layer_idx=cfg.attn_layer_idx,
                            n_heads=cfg.n_heads, n_kv=cfg.n_kv, d_ff=cfg.d_ff, d_state=cfg.d_state,
                            headdim=cfg.headdim, eps=cfg.eps)
    eng = HybridDecoder(ec, W, DEV)
    del W
    utts = list(c["utts"])
    want = [int(s) for s in d["steps"]]
    got = {}

    def record(step):
        if step in want:
            got[step] = eng.last_logits()[utts].cpu().numpy()

    def cb(frame, step, n):
        if frame.shape[2]:
            record(step)
            frame.copy_(hist[..., P + 1 + step:P + 2 + step])
        return step < max(want)

    def after_prefill(frame):
        record(0)
        frame.copy_(hist[..., P + 1:P + 2])

    eng.generate(cond.to(DEV), prefix.to(DEV), T, 2.0, B, CLI_SP, seed=c["seed"], force_full_length=True,
                 callback=cb, _after_prefill=after_prefill)
    assert sorted(got) == want
    ref = d["logits"].astype(np.float32)                        # [U][steps][9][V]
    rows = []
    for j, s in enumerate(want):
        r, g = ref[:, j].copy(), got[s].copy()
        if s == 0:       # the restatement records step 0 after benchmark mode's EOS mask (zonos_ref.generate)
            r[:, 0, 1024] = g[:, 0, 1024] = -np.inf
        fin = np.isfinite(r)
        assert np.array_equal(fin, np.isfinite(g))
        e = np.abs(g[fin] - r[fin])
        rows.append((s, float(e.max()), float(e.mean()), float(np.abs(r[fin]).mean())))
        # greedy-space argmax where the restatement's top-2 gap is clear of the error
        rr, gg = r.copy(), g.copy()
        rr[..., 1024] = gg[..., 1024] = -np.inf
        top = np.sort(rr, axis=-1)[..., -2:]
        ok = (top[..., 1] - top[..., 0]) > 2 * C5_MAX
        assert np.array_equal(rr.argmax(-1)[ok], gg.argmax(-1)[ok]), s
    print("hybrid c5 (step, max |d|, mean |d|, mean |logit|):", rows)
    assert max(r[1] for r in rows) < C5_MAX and max(r[2] for r in rows) < C5_MEAN, rows
    early = np.mean([r[2] for r in rows if r[0] < 3])
    late = np.mean([r[2] for r in rows if r[0] > 2500])
    assert late <= C5_DRIFT * early, (early, late)
