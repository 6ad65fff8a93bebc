"""GPU: every decode-attention entry and the causal prefill against an fp64 reference on inputs in which
single keys matter (tests/attn_probe.py): each (row, head) has a hot key on an edge of the kernels' masks
and key partitions, and every cache position beyond the context is poisoned, so one dropped or one extra
key is an O(1) error. Every comparison is max(|out - ref| / bound) <= 1 with the bound derived in
attn_probe; the ratios are printed (pytest -s), the measured maxima are in profiles/attn_key_tests.txt."""
import pytest
import torch

from zonos_amd import kvlayout as kl

from . import attn_probe as ap
from .attn_probe import PREFILL_S, prefill_future

pytestmark = pytest.mark.gpu
DEV = "cuda"
HD = ap.HD
WS = 8 + 4 * HD                 # work floats per (row, kv head, split)
SLICE_SPLITS = (2, 4, 8, 16)

# (R, H, Hk, ctx, smax, in_proj slabs, NeoX RoPE): the smallest contexts that reach each edge -- one key, the
# 32-key slice (31, 32, 33), a wave's last slice (97), the 128-key block (128, 129), the cache end with no
# tail (255, 256 in 256) and with one (256 in 512), several blocks (300, 1000), 24 blocks (2999: the only
# place 24 splits exist) -- and one cache beyond KV_NT_BYTES (R = 128: the non-temporal instantiation).
# smax 1024 where the context is small lets 3 and 8 splits run there (nsplit <= smax / 128): the splits
# beyond ceil(ctx / 128) are empty, their partials have m = -inf.
CASES = [(2, 16, 4, 1, 256, 4, 0), (3, 2, 1, 31, 256, 1, 1), (2, 16, 4, 32, 1024, 2, 0), (3, 2, 1, 33, 256, 4, 1),
         (2, 16, 4, 97, 1024, 1, 0), (2, 16, 4, 128, 256, 4, 0), (3, 2, 1, 129, 1024, 2, 1), (2, 16, 4, 255, 256, 4, 1),
         (2, 16, 4, 256, 256, 1, 0), (3, 2, 1, 256, 512, 4, 0), (2, 16, 4, 300, 1024, 4, 1), (3, 16, 4, 1000, 1024, 2, 0),
         (2, 16, 4, 2999, 3072, 4, 0), (128, 16, 4, 513, 768, 4, 0)]
IDS = [f"R{c[0]}-H{c[1]}-ctx{c[3]}-smax{c[4]}" for c in CASES]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from zonos_amd import _lib
    _lib.load()


def _nsplits(ctx, smax, least=1):
    """1, 2, 3, 8 (24 at 24 blocks) as far as the cache allows, and one count above the context's blocks."""
    cap, nkb = smax // ap.AT_KB, (ctx + ap.AT_KB - 1) // ap.AT_KB
    ns = {n for n in (1, 2, 3, 8, 24 if nkb == 24 else 1) if n <= cap}
    if nkb < cap:
        ns.add(min(cap, nkb + 1))
    return sorted(n for n in ns if n >= least)


def _i32(x):
    return torch.tensor([x], dtype=torch.int32, device=DEV)


def _nan(*shape, dtype=torch.bfloat16):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _is_sentinel(t):
    return bool(torch.isnan(t).all())


def _report(entry, case, what, ra):
    print(f"ATTN_RATIO {entry:22s} R{case[0]} H{case[1]}/{case[2]} ctx {case[3]} smax {case[4]} {what}: {ra:.3f}")


# ---------------------------------------------------------------------------- shared probes (built once)
_rope = {}


def _fused_inputs(case):
    """The slabs of a fused case and what zk_qkv_rope (pinned to the oracle) makes of them at ctx - 1:
    q, the newest K / V -- once per case, shared by every fused entry."""
    if case not in _rope:
        from zonos_amd._lib import call, ptr, stream_ptr
        from zonos_amd.engine import rope_table
        R, H, Hk, ctx, smax, gs, neox = case
        part = ap.fused_part(R, H, Hk, gs, seed=ctx * 13 + gs, ctx=ctx).to(DEV)
        freqs = rope_table(16384, HD).to(DEV)
        q = _nan(R, H * HD)
        kfull = torch.zeros(R, Hk, smax * HD, dtype=torch.bfloat16, device=DEV)
        vfull = torch.zeros(R, Hk, smax * HD, dtype=torch.bfloat16, device=DEV)
        call("zk_qkv_rope", ptr(part), gs, R, 1, H, Hk, HD, ptr(freqs), ctx - 1, None, ptr(q), ptr(kfull), ptr(vfull),
             smax, None, neox, None, stream_ptr())
        torch.cuda.synchronize()
        knew = kl.unpack_k(kfull.cpu(), smax)[:, :, ctx - 1].clone()
        vnew = kl.unpack_v(vfull.cpu(), smax)[:, :, ctx - 1].clone()
        qc = q.cpu().reshape(R, H, HD)
        # the first head of every group asks for the newest key itself
        assert torch.equal(qc[:, ::H // Hk].view(torch.int16), knew.view(torch.int16))
        _rope[case] = (part, freqs, qc, knew, vnew)
    return _rope[case]


_probes = {}


def _fused_probes(case, fp8):
    key = (case, fp8)
    if key not in _probes:
        R, H, Hk, ctx, smax, gs, neox = case
        _, _, qc, knew, vnew = _fused_inputs(case)
        edges = ap.edge_keys(ctx, _nsplits(ctx, smax))
        _probes[key] = [ap.decode_probe(R, H, Hk, ctx, smax, edges, seed=ctx + 7, rnd=i, q=qc, newest=(knew, vnew),
                                        fp8=fp8) for i in range(ap.n_rounds(edges, R, H, Hk, newest=True))]
    return _probes[key]


def _plain_probes(case, fp8, slice_rule=False):
    key = (case, fp8, slice_rule)
    if key not in _probes:
        R, H, Hk, ctx, smax = case[:5]
        edges = ap.edge_keys(ctx, () if slice_rule else _nsplits(ctx, smax), SLICE_SPLITS if slice_rule else ())
        _probes[key] = [ap.decode_probe(R, H, Hk, ctx, smax, edges, seed=ctx + 3, rnd=i, fp8=fp8)
                        for i in range(ap.n_rounds(edges, R, H, Hk))]
    return _probes[key]


# ---------------------------------------------------------------------------- zk_attn_decode
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_attn_decode_keys(case):
    """Every split count: the output within the bound, with the context as an argument and as 1 + the device
    word (bit-equal); a context one past the cache is the context Smax; a skipped launch writes nothing."""
    from zonos_amd._lib import call, ptr, stream_ptr
    R, H, Hk, ctx, smax = case[:5]
    s = stream_ptr()
    worst = 0.0
    for pr in _plain_probes(case, False):
        qd, kc, vt = pr.q.to(DEV), kl.pack_k(pr.k_in).to(DEV), kl.pack_v(pr.v_in).to(DEV)
        for ns in _nsplits(ctx, smax):
            outs = []
            for ctx0, word in ((ctx, None), (1, _i32(ctx - 1))):
                work, out = _nan(R * Hk * ns * WS, dtype=torch.float32), _nan(R, H * HD)
                call("zk_attn_decode", ptr(qd), ptr(kc), ptr(vt), R, H, Hk, HD, smax, ctx0, ptr(word), ptr(work), ns,
                     ptr(out), None, s)
                torch.cuda.synchronize()
                outs.append(out)
            assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), ns
            ra = pr.ratio(outs[0])
            worst = max(worst, ra)
            assert ra <= 1.0, (ns, ra)
            if ctx == smax:                                   # the clamp: Smax + 1 keys asked for
                for ctx0, word in ((smax + 1, None), (1, _i32(smax))):
                    work, out = _nan(R * Hk * ns * WS, dtype=torch.float32), _nan(R, H * HD)
                    call("zk_attn_decode", ptr(qd), ptr(kc), ptr(vt), R, H, Hk, HD, smax, ctx0, ptr(word), ptr(work),
                         ns, ptr(out), None, s)
                    torch.cuda.synchronize()
                    assert torch.equal(out.view(torch.int16), outs[0].view(torch.int16)), (ns, ctx0)
        ns, skip = _nsplits(ctx, smax)[-1], _i32(1)
        work, out = _nan(R * Hk * ns * WS, dtype=torch.float32), _nan(R, H * HD)
        call("zk_attn_decode", ptr(qd), ptr(kc), ptr(vt), R, H, Hk, HD, smax, ctx, None, ptr(work), ns, ptr(out),
             ptr(skip), s)
        torch.cuda.synchronize()
        assert _is_sentinel(out) and _is_sentinel(work), "a skipped launch wrote"
    _report("zk_attn_decode", case, f"splits {_nsplits(ctx, smax)}", worst)


# ---------------------------------------------------------------------------- the fused entries
def _run_fused(entry, case, ns, part, freqs, kc, vt):
    """One launch of a fused bf16 entry on (kc, vt) -> the attention [R][H][128] (for _part: merged in fp64)."""
    from zonos_amd._lib import call, ptr, stream_ptr
    R, H, Hk, ctx, smax, gs, neox = case
    s = stream_ptr()
    work = _nan(R * Hk * ns * WS, dtype=torch.float32)
    out = _nan(R, H * HD)
    word = _i32(ctx - 1)                                      # ctx = 1 + the device word, as the engine passes it
    if entry == "zk_attn_decode_qkv":
        call(entry, ptr(part), gs, ptr(freqs), ptr(kc), ptr(vt), R, H, Hk, HD, smax, ctx, None, ptr(work), ns, ptr(out),
             neox, None, s)
    elif entry == "zk_attn_decode_qkv_sc":
        cnt = torch.zeros(R * Hk, dtype=torch.int32, device=DEV)
        call(entry, ptr(part), gs, ptr(freqs), ptr(kc), ptr(vt), R, H, Hk, HD, smax, 1, ptr(word), ptr(work), ns, ptr(cnt),
             ptr(out), neox, None, s)
    else:
        call(entry, ptr(part), gs, ptr(freqs), ptr(kc), ptr(vt), R, H, Hk, HD, smax, 1, ptr(word), ptr(work), ns, neox,
             None, s)
    torch.cuda.synchronize()
    return ap.merge_partials(work, R, H, Hk, ns) if entry.endswith("_part") else out


@pytest.mark.parametrize("entry", ["zk_attn_decode_qkv", "zk_attn_decode_qkv_sc", "zk_attn_decode_qkv_part"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_attn_decode_fused_keys(case, entry):
    """The newest key is computed, used from LDS and stored by the kernel: it is the hot key of one head of every
    group, the cache holds poison in its place before the launch. The output within the bound; afterwards the
    cache is the input cache with key ctx - 1 replaced -- the poison tail bit-unchanged."""
    R, H, Hk, ctx, smax, gs, neox = case
    part, freqs = _fused_inputs(case)[:2]
    splits = _nsplits(ctx, smax, least=2 if entry.endswith("_part") else 1)
    worst = 0.0
    for pr in _fused_probes(case, False):
        kc0, vt0 = kl.pack_k(pr.k_in).to(DEV), kl.pack_v(pr.v_in).to(DEV)
        kc1, vt1 = kl.pack_k(pr.k).to(DEV), kl.pack_v(pr.v).to(DEV)
        assert not torch.equal(kc0, kc1)
        for ns in splits:
            kc, vt = kc0.clone(), vt0.clone()
            att = _run_fused(entry, case, ns, part, freqs, kc, vt)
            ra = pr.ratio(att)
            worst = max(worst, ra)
            assert ra <= 1.0, (ns, ra)
            assert torch.equal(kc.view(torch.int16), kc1.view(torch.int16)), ns
            assert torch.equal(vt.view(torch.int16), vt1.view(torch.int16)), ns
            ku, vu = kl.unpack_k(kc.cpu(), smax), kl.unpack_v(vt.cpu(), smax)
            assert torch.equal(ku[:, :, ctx:].view(torch.int16), pr.k_in[:, :, ctx:].view(torch.int16))
            assert torch.equal(vu[:, :, ctx:].view(torch.int16), pr.v_in[:, :, ctx:].view(torch.int16))
    _report(entry, case, f"gs {gs} neox {neox} splits {splits}", worst)


# ---------------------------------------------------------------------------- zk_attn_decode_q_part
@pytest.mark.parametrize("case", CASES[:-1], ids=IDS[:-1])
def test_attn_decode_q_part_keys(case):
    """32-key slices interleaved over 2, 4, 8, 16 workgroups: hot keys on the first and last key of every
    (split, wave) of that rule, the partials merged in fp64; the context as 1 + the device word (the engine's
    form) and as an argument, bit-equal. (A B = 1 path: the R = 128 case is left to the other entries.)"""
    from zonos_amd._lib import call, ptr, stream_ptr
    R, H, Hk, ctx, smax = case[:5]
    s = stream_ptr()
    worst = 0.0
    for pr in _plain_probes(case, False, slice_rule=True):
        qd, kc, vt = pr.q.to(DEV), kl.pack_k(pr.k_in).to(DEV), kl.pack_v(pr.v_in).to(DEV)
        for ns in SLICE_SPLITS:
            works = []
            for ctx0, word in ((1, _i32(ctx - 1)), (ctx, None)):
                work = _nan(R * Hk * ns * WS, dtype=torch.float32)
                call("zk_attn_decode_q_part", ptr(qd), ptr(kc), ptr(vt), R, H, Hk, HD, smax, ctx0, ptr(word), ptr(work),
                     ns, None, s)
                torch.cuda.synchronize()
                works.append(work)
            assert torch.equal(works[0].view(torch.int32), works[1].view(torch.int32)), ns
            ra = pr.ratio(ap.merge_partials(works[0], R, H, Hk, ns))
            worst = max(worst, ra)
            assert ra <= 1.0, (ns, ra)
        work, skip = _nan(R * Hk * 16 * WS, dtype=torch.float32), _i32(1)
        call("zk_attn_decode_q_part", ptr(qd), ptr(kc), ptr(vt), R, H, Hk, HD, smax, ctx, None, ptr(work), 16,
             ptr(skip), s)
        torch.cuda.synchronize()
        assert _is_sentinel(work), "a skipped launch wrote"
    _report("zk_attn_decode_q_part", case, f"splits {list(SLICE_SPLITS)}", worst)


# ---------------------------------------------------------------------------- the FP8 cache
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_attn_decode_f8_keys(case):
    """The probe cache quantised with kvlayout.quantize_kv_e4m3; reference and bound on the dequantised values
    (power-of-two scales: exact, the bound is unchanged); p(j*) >= 0.5 re-asserted by the helper."""
    from zonos_amd._lib import call, ptr, stream_ptr
    R, H, Hk, ctx, smax = case[:5]
    s = stream_ptr()
    worst = 0.0
    for pr in _plain_probes(case, True):
        z = pr.quant
        qd, k8, v8 = pr.q.to(DEV), kl.pack_k8(z["kq"]).to(DEV), kl.pack_v8(z["vq"]).to(DEV)
        ksd, vsd = z["ks"].contiguous().to(DEV), z["vs"].contiguous().to(DEV)
        for ns in _nsplits(ctx, smax):
            work, out, word = _nan(R * Hk * ns * WS, dtype=torch.float32), _nan(R, H * HD), _i32(ctx - 1)
            call("zk_attn_decode_f8", ptr(qd), ptr(k8), ptr(v8), ptr(ksd), ptr(vsd), R, H, Hk, HD, smax, 1,
                 ptr(word), ptr(work), ns, ptr(out), None, s)
            torch.cuda.synchronize()
            ra = pr.ratio(out)
            worst = max(worst, ra)
            assert ra <= 1.0, (ns, ra)
    _report("zk_attn_decode_f8", case, f"splits {_nsplits(ctx, smax)}", worst)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_attn_decode_qkv_f8_keys(case):
    """The fused FP8 entry (splits combined by k_attn_combine and, with counters, in the launch): the output
    within the bound of the dequantised cache whose key ctx - 1 is the quantised newest key; afterwards the byte
    caches and scales are the input's with that key replaced, the poison tail bit-unchanged."""
    from zonos_amd._lib import call, ptr, stream_ptr
    R, H, Hk, ctx, smax, gs, neox = case
    if neox:
        case = (R, H, Hk, ctx, smax, gs, 0)                   # (the FP8 entry has the interleaved RoPE only)
    part, freqs = _fused_inputs(case)[:2]
    s = stream_ptr()
    worst = 0.0
    for pr in _fused_probes(case, True):
        z = pr.quant
        dev = {n: (kl.pack_k8(t) if n[0] == "k" and n[1] == "q" else kl.pack_v8(t) if n[:2] == "vq" else t)
               .contiguous().to(DEV) for n, t in z.items()}
        for ns in _nsplits(ctx, smax):
            for counters in (False, True):
                k8, v8, ksd, vsd = (dev[n].clone() for n in ("kq", "vq", "ks", "vs"))
                work, out = _nan(R * Hk * ns * WS, dtype=torch.float32), _nan(R, H * HD)
                cnt = torch.zeros(R * Hk, dtype=torch.int32, device=DEV) if counters else None
                word = _i32(ctx - 1)
                call("zk_attn_decode_qkv_f8", ptr(part), gs, ptr(freqs), ptr(k8), ptr(v8), ptr(ksd), ptr(vsd), R, H, Hk,
                     HD, smax, 1, ptr(word), ptr(work), ns, ptr(cnt), ptr(out), None, s)
                torch.cuda.synchronize()
                ra = pr.ratio(out)
                worst = max(worst, ra)
                assert ra <= 1.0, (ns, counters, ra)
                assert torch.equal(k8, dev["kq_ref"]) and torch.equal(ksd, dev["ks_ref"]), (ns, counters)
                assert torch.equal(v8, dev["vq_ref"]) and torch.equal(vsd, dev["vs_ref"]), (ns, counters)
                assert torch.equal(kl.unpack_k8(k8.cpu(), smax)[:, :, ctx:], z["kq"][:, :, ctx:])
                assert torch.equal(kl.unpack_v8(v8.cpu(), smax)[:, :, ctx:], z["vq"][:, :, ctx:])
                assert torch.equal(ksd.cpu()[:, :, ctx:], z["ks"][:, :, ctx:])
                assert torch.equal(vsd.cpu()[:, :, ctx:], z["vs"][:, :, ctx:])
    _report("zk_attn_decode_qkv_f8", case, f"gs {gs} splits {_nsplits(ctx, smax)}", worst)


# ---------------------------------------------------------------------------- zk_attn_prefill
@pytest.mark.parametrize("R,H,Hk", [(2, 16, 4), (3, 2, 1)])
@pytest.mark.parametrize("S", PREFILL_S)
def test_attn_prefill_causal_keys(S, R, H, Hk):
    """The 16-query wave, 64-query workgroup and 32-key slice edges: hot keys on the diagonal, on key 0 and on
    the first key of the query's slice; a cache one 32-key chunk longer than S, poisoned; future-hot keys right
    after the last query of a wave / slice / workgroup."""
    from zonos_amd._lib import call, ptr, stream_ptr
    smax = (S + 31) // 32 * 32 + 32
    for fut in ((), prefill_future(S)):
        pp = ap.prefill_probe(R, S, H, Hk, smax, seed=S + H, future=fut)
        qd = pp.q.reshape(R * S, H * HD).contiguous().to(DEV)
        kc, vt = kl.pack_k(pp.k).to(DEV), kl.pack_v(pp.v).to(DEV)
        out = _nan(R * S, H * HD)
        call("zk_attn_prefill", ptr(qd), ptr(kc), ptr(vt), R, S, H, Hk, HD, smax, ptr(out), stream_ptr())
        torch.cuda.synchronize()
        ra = pp.ratio(out)
        print(f"ATTN_RATIO zk_attn_prefill        R{R} H{H}/{Hk} S {S} smax {smax} future {list(fut)}: {ra:.3f}")
        assert ra <= 1.0, (list(fut), ra)
