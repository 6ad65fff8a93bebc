"""GPU: ragged request batches -- conditionings of different lengths, every row at its own KV position and context.

(a) zk_attn_decode_qkv_sc_rows and (b) zk_attn_decode_qkv_f8_rows against the uniform entry run once per distinct
context; (c) the prefill placement (zk_embed_codes_rows) and the last-valid-position gather; (d) every request of a
tiny ragged batch equals generate() of it alone at B = 1; (e) at full width a request's codes do not depend on the
longest conditioning of its batch; (f) nor on what the padding holds; (g) two ranks sharing the GPU; (h) the engine
returns to the uniform path. Every comparison is bit for bit."""
import ctypes as C
import os
import socket

import pytest
import torch

from zonos_amd import kvlayout as kl
from zonos_amd.requests import Request

from .golden_util import TINY, load_gen_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
HD = 128
GREEDY = dict(temperature=0.0, top_p=0, top_k=0, min_p=0, linear=0.0, conf=0.0, quad=0.0, repetition_penalty=1.0,
              repetition_penalty_window=2)

# ---------------------------------------------------------------------------- (a), (b) the attention kernels
R_, H_, HK_, SMAX_ = 8, 8, 2, 512
CTX_WORD = 300                                                # *ctx_dev, ctx0 = 1: the uniform context is 301
ROW_OFF = [0, -1, -12, -44, -172, -173, -268, -300]
CTXS = [301, 300, 289, 257, 129, 128, 33, 1]                  # last key in a new 32-key slice, a slice exactly
#                                                               full, a new 128-key block, a full block, one key
POISON = 1e30


def _attn_inputs(gs, seed):
    """Random slabs and RoPE table; per row random keys below its own context and +-1e30 from ctx_r - 1 on (the
    slot of the new key and everything behind it), unpacked bf16 [R][Hk][Smax][128]."""
    assert [1 + CTX_WORD + o for o in ROW_OFF] == CTXS
    g = torch.Generator().manual_seed(seed)
    N = (H_ + 2 * HK_) * HD
    part = torch.randn(gs, R_, N, generator=g) * 0.5
    freqs = torch.randn(SMAX_, HD // 2, 2, generator=g)       # random per position: a wrong RoPE row shows
    k = torch.randn(R_, HK_, SMAX_, HD, generator=g)
    v = torch.randn(R_, HK_, SMAX_, HD, generator=g)
    sign = torch.where(torch.rand(R_, HK_, SMAX_, HD, generator=g) < 0.5, -1.0, 1.0)
    for r, c in enumerate(CTXS):
        k[r, :, c - 1:] = POISON * sign[r, :, c - 1:]
        v[r, :, c - 1:] = -POISON * sign[r, :, c - 1:]
    return part.to(DEV), freqs.contiguous().to(DEV), k.to(torch.bfloat16), v.to(torch.bfloat16)


def _word(v):
    return torch.tensor([v], dtype=torch.int32, device=DEV)


def _run_attn(fp8, caches, part, freqs, gs, nsplit, counters, ctx_word, row_off):
    """One launch on clones of `caches` (device, packed): bf16 (kc, vt) or FP8 (k8, v8, ksc, vsc). row_off None:
    the uniform entry. Returns (out, caches after)."""
    from zonos_amd._lib import call, ptr, stream_ptr
    cs = [c.clone() for c in caches]
    work = torch.zeros(R_ * HK_ * nsplit * (8 + 4 * HD), device=DEV)
    cnt = torch.zeros(R_ * HK_, dtype=torch.int32, device=DEV) if counters else None
    out = torch.full((R_, H_ * HD), 7.0, dtype=torch.bfloat16, device=DEV)
    cw = _word(ctx_word)
    head = (ptr(part), gs, ptr(freqs), *[ptr(c) for c in cs], R_, H_, HK_, HD, SMAX_, 1, ptr(cw))
    tail = (ptr(work), nsplit, ptr(cnt), ptr(out))
    name = "zk_attn_decode_qkv_f8" if fp8 else "zk_attn_decode_qkv_sc"
    if row_off is not None:
        call(name + "_rows", *head, ptr(row_off), *tail, None, stream_ptr())
    elif fp8:
        call(name, *head, *tail, None, stream_ptr())
    else:
        call(name, *head, *tail, 0, None, stream_ptr())
    torch.cuda.synchronize()
    return out, cs


def _check_rows_attention(fp8, gs, nsplit, counters):
    from zonos_amd._lib import call, ptr, stream_ptr
    part, freqs, k, v = _attn_inputs(gs, seed=17 * gs + nsplit)
    kc, vt = kl.pack_k(k).to(DEV), kl.pack_v(v).to(DEV)
    if fp8:                                                   # the caches as the prefill leaves them
        k8, v8 = (torch.zeros(R_, HK_, SMAX_ * HD, dtype=torch.uint8, device=DEV) for _ in range(2))
        ksc, vsc = (torch.zeros(R_, HK_, SMAX_, dtype=torch.uint8, device=DEV) for _ in range(2))
        call("zk_kv_quantize_e4m3", ptr(kc), ptr(vt), R_, HK_, HD, SMAX_, SMAX_, ptr(k8), ptr(v8), ptr(ksc), ptr(vsc),
             SMAX_, stream_ptr())
        torch.cuda.synchronize()
        caches = [k8, v8, ksc, vsc]
    else:
        caches = [kc.contiguous(), vt.contiguous()]
    caches = [c.view(R_, -1) for c in caches]                 # [R][...]: a row's whole cache (or scale array)
    ro = torch.tensor(ROW_OFF, dtype=torch.int32, device=DEV)
    got, got_c = _run_attn(fp8, caches, part, freqs, gs, nsplit, counters, CTX_WORD, ro)
    uni301, _ = _run_attn(fp8, caches, part, freqs, gs, nsplit, counters, CTX_WORD, None)
    differs = 0
    for c in sorted(set(CTXS)):
        exp, exp_c = _run_attn(fp8, caches, part, freqs, gs, nsplit, counters, c - 1, None)
        for r in (r for r, cr in enumerate(CTXS) if cr == c):
            assert torch.isfinite(exp[r].float()).all(), (c, r)
            assert torch.equal(got[r], exp[r]), (c, r, (got[r].float() - exp[r].float()).abs().max())
            for i, (a, b) in enumerate(zip(got_c, exp_c)):    # the new key landed at ctx_r - 1 and nowhere else
                assert torch.equal(a[r], b[r]), (c, r, i)
                assert not torch.equal(a[r], caches[i][r]), (c, r, i)
            differs += int(not torch.equal(uni301[r], exp[r]))
    assert differs >= 6, differs                              # not vacuous: the uniform context is wrong for them
    # row_off all zero is the uniform entry
    z, z_c = _run_attn(fp8, caches, part, freqs, gs, nsplit, counters, CTX_WORD, torch.zeros_like(ro))
    u, u_c = _run_attn(fp8, caches, part, freqs, gs, nsplit, counters, CTX_WORD, None)
    assert torch.equal(z.view(torch.int16), u.view(torch.int16))      # (rows read poison here: compare the bits)
    assert all(torch.equal(a, b) for a, b in zip(z_c, u_c))


@pytest.mark.parametrize("counters", [False, True])
@pytest.mark.parametrize("nsplit", [1, 2, 4])
@pytest.mark.parametrize("gs", [1, 2])
def test_attention_rows_equals_uniform_per_context(gs, nsplit, counters):
    _check_rows_attention(False, gs, nsplit, counters)


@pytest.mark.parametrize("nsplit", [1, 2])
@pytest.mark.parametrize("gs", [1, 2])
def test_attention_rows_f8_equals_uniform_per_context(gs, nsplit):
    _check_rows_attention(True, gs, nsplit, True)


# ---------------------------------------------------------------------------- (c) prefill placement and gather
@pytest.mark.parametrize("D", [2048, TINY.d_model])
def test_prefill_placement_and_last_position_gather(D):
    from zonos_amd._lib import call, ptr, stream_ptr
    B, P, K, V, Ld = 3, 2, 9, 1026, 20
    lens = (5, 9, 7)
    Lc, S1 = max(lens), P + 1
    S = Lc + S1
    g = torch.Generator().manual_seed(D)
    emb = (torch.randn(K, V, D, generator=g) * 0.3).to(torch.bfloat16).to(DEV)
    ids = torch.randint(0, V, (B, K, Ld), generator=g).to(DEV)
    ro = torch.tensor([n - Lc for n in lens] * 2, dtype=torch.int32, device=DEV)
    fill = torch.tensor(3.0, dtype=torch.bfloat16)
    x = torch.full((2 * B, S, D), 3.0, dtype=torch.bfloat16, device=DEV)
    s = stream_ptr()
    call("zk_embed_codes_rows", ptr(ids), B, S1, K, K * Ld, Ld, ptr(emb), V, D, 2, ptr(x), S, Lc, ptr(ro), s)
    torch.cuda.synchronize()
    for r in range(2 * B):
        b, n = r % B, lens[r % B]
        # zk_embed_codes of the row alone ...
        ref = torch.empty(1, S1, D, dtype=torch.bfloat16, device=DEV)
        call("zk_embed_codes", ptr(ids[b]), 1, S1, K, K * Ld, Ld, None, 0, ptr(emb), V, D, 1, ptr(ref), S1, 0, None,
             None, 1e-5, None, None, s)
        torch.cuda.synchronize()
        assert torch.equal(x[r, n:n + S1], ref[0]), r
        # ... and torch indexing of the same sum (bf16 adds left to right, model.py:97-98)
        acc = emb[0][ids[b, 0, :S1]]
        for k in range(1, K):
            acc = acc + emb[k][ids[b, k, :S1]]
        assert torch.equal(x[r, n:n + S1], acc), r
        assert (x[r, :n].cpu() == fill).all() and (x[r, n + S1:].cpu() == fill).all(), r      # nothing else written
    # the gather: each row's last valid position, S_r - 1 = Lc_r + P
    xn = torch.randn(2 * B, S, D, generator=g).to(torch.bfloat16).to(DEV)
    out = torch.zeros(2 * B, D, dtype=torch.bfloat16, device=DEV)
    call("zk_gather_last_rows", ptr(xn), 2 * B, S, D, ptr(ro), ptr(out), s)
    torch.cuda.synchronize()
    for r in range(2 * B):
        assert torch.equal(out[r], xn[r, lens[r % B] + S1 - 1]), r
    # offsets out of range are clamped into the row on the device (device data cannot be validated by the entry)
    bad = torch.tensor([-1000, 1000] * B, dtype=torch.int32, device=DEV)
    call("zk_gather_last_rows", ptr(xn), 2 * B, S, D, ptr(bad), ptr(out), s)
    x2 = torch.full((2 * B, S, D), 3.0, dtype=torch.bfloat16, device=DEV)
    call("zk_embed_codes_rows", ptr(ids), B, S1, K, K * Ld, Ld, ptr(emb), V, D, 2, ptr(x2), S, Lc, ptr(bad), s)
    torch.cuda.synchronize()
    for r in range(2 * B):
        assert torch.equal(out[r], xn[r, 0 if r % 2 == 0 else S - 1]), r
        t0 = 0 if r % 2 == 0 else S - S1
        assert torch.equal(x2[r, t0:t0 + S1], x[r, lens[r % B]:lens[r % B] + S1]), r


# ---------------------------------------------------------------------------- (d) a request in a ragged batch == alone
def _tiny_engine(W):
    from zonos_amd.engine import EngineConfig, HipDecoder
    return HipDecoder(EngineConfig(TINY.d_model, TINY.n_layer, TINY.n_heads, TINY.n_kv, TINY.d_ff, TINY.eps), W, DEV)


def _utt(c, b):
    B = c["B"]
    return torch.stack([c["cond"][b], c["cond"][B + b]]), c["prefix"][b]


# conditioning lengths of the five requests: the fixture's Lc = 12 kept once, 7 loses more than a third of it
RAGGED_LC = (12, 9, 7, 11, 10)


def ragged_requests(c, knobs_sp):
    """test_gpu_requests.mixed_requests -- the three eos_sampled utterances as that fixture runs them (seed 1234, keys
    0, 1, 2), one request with the sampled_knobs parameters, another seed and cfg_scale 3, and one greedy request
    with a budget of 5 -- each conditioning truncated to its RAGGED_LC tokens."""
    reqs = [Request(*_utt(c, b), c["max_new"], 2.0, c["sp"], c["seed"], b) for b in range(3)]
    reqs.append(Request(*_utt(c, 1), c["max_new"], 3.0, knobs_sp, 77, 5))
    reqs.append(Request(*_utt(c, 2), 5, 2.0, GREEDY, 3, 9))
    Lc = c["cond"].shape[1]
    assert max(RAGGED_LC) == Lc and len(set(RAGGED_LC)) == 5 and min(RAGGED_LC) <= 2 * Lc // 3
    for r, n in zip(reqs, RAGGED_LC):
        r.conditioning = r.conditioning[:, :n].contiguous()
    return reqs


def _alone(eng, r, **kw):
    """generate() of one request at B = 1: its arguments, row_base = its key."""
    return eng.generate(r.conditioning.to(DEV), r.audio_prefix_codes[None].to(DEV), r.max_new_tokens, r.cfg_scale, 1,
                        r.sampling_params, seed=r.seed, row_base=r.key, force_full_length=r.force_full_length,
                        **kw)[0].cpu()


@pytest.fixture(scope="module")
def ragged():
    c = load_gen_case("eos_sampled")
    reqs = ragged_requests(c, load_gen_case("sampled_knobs")["sp"])
    eng = _tiny_engine(c["W"])
    return dict(c=c, reqs=reqs, eng=eng, alone=[_alone(eng, r) for r in reqs])


def _prefill_path(M):
    """The GEMM family of a prefill GEMM over M rows (gemm.hip gemm_plan): distributed.gemm_regime's thresholds."""
    return "gemv" if M <= 16 else ("ws" if M <= 128 else "gemm")


@pytest.mark.parametrize("c_step", [True, False])
@pytest.mark.parametrize("use_graph", [True, False])
def test_request_in_ragged_batch_equals_request_alone(ragged, use_graph, c_step, monkeypatch):
    """One regime for the decode GEMMs and the attention split. The prefill GEMMs cannot share a family here: a
    request alone runs 2 S_b <= 34 rows (k_gemm_ws), the batch 2 B S = 170 rows (k_gemm), exactly as in
    test_gpu_requests' uniform batch of the same five requests -- both families accumulate a row's K chunks in
    order in one split, and the comparison below stays bit for bit; test (e) compares within one family."""
    from zonos_amd.distributed import gemm_regime
    from zonos_amd.engine import ATTN_CHUNK, HipDecoder, attn_splits_for
    reqs, eng, alone = ragged["reqs"], ragged["eng"], ragged["alone"]
    lens = [int(a.shape[1]) for a in alone]
    budgets = [r.max_new_tokens for r in reqs]
    print("B = 1 lengths", lens, "budgets", budgets)
    by_eos = sorted(n for n, m in zip(lens, budgets) if n < m)
    assert len(set(by_eos)) >= 2, lens                        # two requests end by EOS at different steps
    B, P = len(reqs), ragged["c"]["prefix"].shape[2]
    assert B <= 8 and gemm_regime(B) == gemm_regime(1)
    smax = [-(-(lc + P + n + 9) // ATTN_CHUNK) * ATTN_CHUNK for lc, n in zip(RAGGED_LC, budgets)]
    smax.append(-(-(max(RAGGED_LC) + P + max(budgets) + 9) // ATTN_CHUNK) * ATTN_CHUNK)
    assert len({attn_splits_for(2 * b, TINY.n_kv, s) for b in (B, 1) for s in smax}) == 1
    S = max(RAGGED_LC) + P + 1
    assert {_prefill_path(2 * (lc + P + 1)) for lc in RAGGED_LC} == {"ws"} and _prefill_path(2 * B * S) == "gemm"
    monkeypatch.setattr(HipDecoder, "c_step", c_step)
    got = eng.generate_requests(reqs, use_graph=use_graph, poll_every=7, ragged=True)
    assert eng._ws["rows"] is not None and eng._ws["row_off"] is not None and len(got) == B
    assert eng._ws["row_off"].tolist() == [n - max(RAGGED_LC) for n in RAGGED_LC] * 2
    for b, (x, a) in enumerate(zip(got, alone)):
        assert x.shape == a.shape and torch.equal(x.cpu(), a), (b, x.shape, a.shape)


# ---------------------------------------------------------------------------- (f) what the padding holds
@pytest.mark.parametrize("c_step", [True, False])
def test_pad_content_does_not_matter(ragged, c_step, monkeypatch):
    """1e4 in place of zero in every pad position of the conditioning (both paths) and of x behind it (the prefill
    this class issues itself; zk_prefill_rows zeroes those): the same codes."""
    from zonos_amd.engine import HipDecoder
    monkeypatch.setattr(HipDecoder, "c_step", c_step)
    got = ragged["eng"].generate_requests(ragged["reqs"], poll_every=7, ragged=True, _pad_fill=1e4)
    for b, (x, a) in enumerate(zip(got, ragged["alone"])):
        assert x.shape == a.shape and torch.equal(x.cpu(), a), (b, x.shape, a.shape)


# ---------------------------------------------------------------------------- (h) back to the uniform path
def test_uniform_calls_after_a_ragged_one(ragged):
    eng, c = ragged["eng"], ragged["c"]
    full = [Request(*_utt(c, b), 12, 2.0, c["sp"], c["seed"], b) for b in range(3)]
    before = [x.cpu() for x in eng.generate_requests(full, poll_every=7)]
    one = _alone(eng, full[1])
    key_uniform = eng._ws["key"]
    # the same B, Lc (the longest), P and budget as `full`, ragged: another workspace key
    rag = [Request(r.conditioning[:, :12 - 3 * b].contiguous(), r.audio_prefix_codes, 12, 2.0, c["sp"], c["seed"], b)
           for b, r in enumerate(full)]
    eng.generate_requests(full, poll_every=7)
    key_full = eng._ws["key"]
    got = eng.generate_requests(rag, poll_every=7, ragged=True)
    assert eng._ws["key"] != key_full and eng._ws["row_off"] is not None and key_uniform != key_full
    assert torch.equal(got[0].cpu(), before[0])               # request 0 kept its conditioning
    after = [x.cpu() for x in eng.generate_requests(full, poll_every=7)]
    assert eng._ws["row_off"] is None and eng._ws["key"] == key_full
    assert all(torch.equal(x, y) for x, y in zip(before, after))
    assert torch.equal(_alone(eng, full[1]), one) and eng._ws["rows"] is None and eng._ws["row_off"] is None
    # ragged=True with equal lengths is the uniform path
    same = [x.cpu() for x in eng.generate_requests(full, poll_every=7, ragged=True)]
    assert eng._ws["row_off"] is None and all(torch.equal(x, y) for x, y in zip(before, same))


# ---------------------------------------------------------------------------- (e) full width
FULL_CFG = dict(d_model=2048, n_layer=2, n_heads=16, n_kv=4, d_ff=2048)
PARAM_POOL = [
    dict(linear=0.65, conf=0.4, quad=0.0, repetition_penalty=2.5, repetition_penalty_window=8, temperature=1.0),
    dict(top_p=0.9, top_k=50, min_p=0.05, linear=0.0, repetition_penalty=1.5, repetition_penalty_window=4,
         temperature=0.8),
    GREEDY,
    dict(temperature=1.2, linear=0.0, top_k=20, repetition_penalty=3.0, repetition_penalty_window=2),
]


@pytest.fixture(scope="module")
def full_engine():
    from zonos_amd.engine import EngineConfig, HipDecoder
    from zonos_amd.synthetic import backbone_weights
    return HipDecoder(EngineConfig(**FULL_CFG), backbone_weights(DEV, seed=4, **FULL_CFG), DEV)


def _pool_lc(i):
    return 4 + (3 * i) % 9                                     # 4, 7, 10, 4, ...


def _pool_request(i):
    from zonos_amd.synthetic import conditioning
    cond = conditioning(1, _pool_lc(i), FULL_CFG["d_model"], seed=100 + i)
    return Request(cond, None, 14 + (5 * i) % 11, (2.0, 3.0, 1.5)[i % 3], PARAM_POOL[i % 4], seed=1000 + 7 * i,
                   key=50 + 3 * i, force_full_length=i % 5 == 4)


@pytest.mark.parametrize("B,kw", [(12, {}), (3, {}), (12, dict(kv_dtype="fp8")), (3, dict(weight_dtype="fp8"))],
                         ids=["B12", "B3", "B12-kv8", "B3-w8"])
def test_longest_conditioning_of_the_batch_does_not_matter_full_width(full_engine, B, kw):
    """Two ragged batches share half of their requests (two of three at B = 3) in other slots; the first holds no
    request of length 10, so the common requests run under Lc_max 7 and 10, i.e. under different row_off."""
    from zonos_amd.distributed import gemm_regime
    short = [i for i in range(3 * B) if _pool_lc(i) < 10]      # lengths 4 and 7 only
    long_ = [i for i in range(3 * B) if _pool_lc(i) == 10]
    first = short[:B]
    common = first[:B // 2] if B > 3 else first[:2]
    second = common[::-1] + long_[:B - len(common)]
    second = second[1::2] + second[0::2] if B > 3 else second[2:] + second[:2]
    pool = {i: _pool_request(i) for i in set(first + second)}
    lc_a, lc_b = max(_pool_lc(i) for i in first), max(_pool_lc(i) for i in second)
    assert (lc_a, lc_b) == (7, 10) and len({_pool_lc(i) for i in common}) == 2
    assert any(first.index(i) != second.index(i) for i in common)
    # one family for the prefill GEMMs of both batches (and one decode regime: the same B)
    assert _prefill_path(2 * B * (lc_a + 1)) == _prefill_path(2 * B * (lc_b + 1)) and gemm_regime(B) == gemm_regime(B)
    a = full_engine.generate_requests([pool[i] for i in first], poll_every=8, ragged=True, **kw)
    assert full_engine._ws["row_off"] is not None
    b = full_engine.generate_requests([pool[i] for i in second], poll_every=8, ragged=True, **kw)
    assert len(a) == len(b) == B and len({x.shape[1] for x in a}) > 1
    for i in common:
        x, y = a[first.index(i)], b[second.index(i)]
        assert x.shape == y.shape and x.shape[1] > 0 and torch.equal(x, y), (i, x.shape, y.shape)


@pytest.mark.parametrize("B,kw", [(12, {}), (3, {}), (12, dict(kv_dtype="fp8")), (3, dict(weight_dtype="fp8"))],
                         ids=["B12", "B3", "B12-kv8", "B3-w8"])
def test_python_sequence_equals_c_step_full_width(full_engine, B, kw, monkeypatch):
    """The Python-issued sequence (c_step False: _layers at B = 12, _layers_small at B = 3, the prefill branch of
    _begin) is the C step's reference: the same ragged batch gives the same codes through both, graph and eager.
    (Test (d) reaches _layers only: the tiny model never takes the five-launch path.)"""
    from zonos_amd.engine import HipDecoder
    reqs = [_pool_request(i) for i in range(B)]
    assert len({_pool_lc(i) for i in range(B)}) == 3
    ref = [x.cpu() for x in full_engine.generate_requests(reqs, poll_every=8, ragged=True, **kw)]
    assert full_engine._small(2 * B) == (B == 3)              # the five-launch path at B = 3, seven launches at 12
    assert len({x.shape[1] for x in ref}) > 1 and all(x.shape[1] > 0 for x in ref)
    monkeypatch.setattr(HipDecoder, "c_step", False)
    for use_graph in (True, False):
        got = full_engine.generate_requests(reqs, poll_every=8, ragged=True, use_graph=use_graph, **kw)
        assert full_engine._ws["row_off"] is not None
        for b, (x, y) in enumerate(zip(got, ref)):
            assert x.shape == y.shape and torch.equal(x.cpu(), y), (use_graph, b, x.shape, y.shape)


# ---------------------------------------------------------------------------- (g) two ranks on the one GPU
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, world, port, q):
    try:
        import torch.distributed as dist

        from zonos_amd.distributed import generate_sharded_requests
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
        c = load_gen_case("eos_sampled")
        reqs = ragged_requests(c, load_gen_case("sampled_knobs")["sp"])
        eng = _tiny_engine(c["W"])
        local, allc = generate_sharded_requests(eng, reqs, coll_device="cpu", return_local=True, poll_every=5,
                                                ragged=True)
        shard_lc = eng._ws["key"][1]                           # the shard planned its own longest conditioning
        one = eng.generate_requests(reqs, poll_every=5, ragged=True)
        ok = len(allc) == len(reqs) and all(x.shape == y.shape and torch.equal(x.cpu(), y.cpu())
                                            for x, y in zip(allc, one))
        q.put((rank, ok, len(local), [int(x.shape[1]) for x in allc], shard_lc))
        dist.destroy_process_group()
    except Exception as e:       # report instead of hanging the parent
        q.put((rank, False, -1, repr(e), None))


def test_generate_sharded_ragged_requests_two_ranks():
    """Five ragged requests over two ranks (3 + 2, the short shard padded): the gathered codes are one process's."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = sorted(q.get(timeout=240) for _ in ps)
    for p in ps:
        p.join(timeout=60)
    assert all(r[1] for r in res), res
    assert [r[2] for r in res] == [3, 2], res
    assert [r[4] for r in res] == [max(RAGGED_LC[:3]), max(RAGGED_LC[3:])], res
