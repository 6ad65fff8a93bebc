"""GPU: request batches -- per-utterance sampling parameters, CFG scale, seed, noise key and budget, rows independent.

(a) zk_sample_heads_rows alone against zk_sample_heads run once per row with that row's parameters;
(b) every request of a mixed batch (EOS at different steps, a spent budget) equals generate() of it alone at B = 1;
(c) at full width a request's codes do not depend on its neighbours, its slot or the dtype options' regime;
(d) the hybrid engine; (e) two ranks sharing the GPU; (f) uniform parameters equal generate(force_full_length).
Every comparison is bit for bit: a request in a batch runs the arithmetic it runs alone (one kernel regime)."""
import ctypes as C
import os
import socket

import pytest
import torch

from zonos_amd.requests import Request

from .golden_util import TINY, load_gen_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
GREEDY = dict(temperature=0.0, top_p=0, top_k=0, min_p=0, linear=0.0, conf=0.0, quad=0.0, repetition_penalty=1.0,
              repetition_penalty_window=2)


# ---------------------------------------------------------------------------- (a) the sampler kernel alone
HEADS_SETS = [
    # (sampling parameters, repetition penalty in effect, cfg_scale)
    (dict(temperature=0.0, rp_window=2), 1.0, 2.0),                                             # greedy
    (dict(temperature=1.0, top_p=0.9, top_k=50, min_p=0.05, rp_window=2), 1.0, 3.0),
    (dict(temperature=1.0, linear=0.65, conf=0.4, quad=0.1, rp_window=2), 1.0, 2.0),            # unified
    (dict(temperature=0.9, rp_window=6), 5.0, 3.0),                                             # penalty, window 6
]
HEADS_SEEDS = [11, 2 ** 40 + 5, 77, 1234]
HEADS_KEYS = [4, 9, 6, 300]                  # all >= B


def _sp(d, cfg):
    from zonos_amd._lib import SamplingParams
    return SamplingParams(d.get("temperature", 1.0), d.get("top_p", 0.0), d.get("min_p", 0.0), d.get("linear", 0.0),
                          d.get("conf", 0.0), d.get("quad", 0.0), d.get("top_k", 0), d["rp_window"], cfg, 0)


@pytest.mark.parametrize("nsplit", [1, 2])
def test_sample_heads_rows_equals_sample_heads_per_row(nsplit):
    from zonos_amd import _lib
    from zonos_amd._lib import GenState, RowParams, call, ptr
    B, K, V, Ld, OFF, STEP = 4, 9, 1026, 32, 20, 5
    g = torch.Generator().manual_seed(nsplit)
    # unit-variance logits per CFG half (summed over the slabs): flat enough that a sampled row is not the argmax
    part = torch.randn(nsplit, 2 * B, K * V, generator=g) / nsplit ** 0.5
    hist = torch.randint(0, 1024, (B, K, Ld), generator=g)
    # row 3's window (the last 6 of the OFF history columns) holds the tokens that would otherwise win: logit 30
    # on both CFG halves (CFG leaves it 30; every other logit has sigma 4.4, so stays below ~18). Unpenalised they
    # take all the mass; divided by the penalty 5 they fall to 6, below the top of the others.
    hot = torch.randint(0, 1024, (K, 6), generator=g)
    hist[3, :, OFF - 6:OFF] = hot
    for k in range(K):
        part[:, 3, k * V + hot[k]] = 0.0
        part[:, B + 3, k * V + hot[k]] = 0.0
        part[0, 3, k * V + hot[k]] = 30.0
        part[0, B + 3, k * V + hot[k]] = 30.0
    part, hist = part.to(DEV), hist.to(DEV)
    i32 = dict(dtype=torch.int32, device=DEV)
    scal = torch.tensor([OFF, 40, STEP, 0, 0, 100] + [0] * 10, **i32)
    zeros = torch.zeros(B, **i32)
    act = torch.tensor([0, 1, 0, 0], **i32)                   # row 1 inside its EOS hold-off
    rp = torch.tensor([s[1] for s in HEADS_SETS], device=DEV)
    stream = _lib.stream_ptr(DEV)

    def state(seed, row_base, tok0, rp_t=rp):
        return GenState(ptr(scal), ptr(zeros), ptr(zeros), ptr(zeros), ptr(zeros), ptr(act), ptr(rp_t), ptr(tok0),
                        ptr(tok0), ptr(hist), B, K, Ld, V, seed, row_base, 0, 0, 0, 0)

    rows = (RowParams * B)(*[RowParams(_sp(d, cfg), HEADS_SEEDS[b], HEADS_KEYS[b], 0)
                             for b, (d, _, cfg) in enumerate(HEADS_SETS)])
    rows_dev = torch.frombuffer(bytearray(bytes(rows)), dtype=torch.uint8).to(DEV)
    for prefill in (0, 1):
        got = torch.full((B * K,), -1, **i32)
        st = state(999, 0, got)                               # st.seed / st.row_base are not read
        dbg_r = torch.zeros(B, K, V, device=DEV)
        call("zk_sample_heads_rows", ptr(part), nsplit, C.byref(st), ptr(rows_dev), prefill, 0, ptr(dbg_r), stream)
        torch.cuda.synchronize()
        got = got.view(B, K).cpu()
        ref = []                                              # ref[p][r]: row r sampled with row p's parameters
        for b, (d, _, cfg) in enumerate(HEADS_SETS):
            tok = torch.full((B * K,), -1, **i32)
            sp, st = _sp(d, cfg), state(HEADS_SEEDS[b], HEADS_KEYS[b] - b, tok)
            dbg = torch.zeros(B, K, V, device=DEV)
            call("zk_sample_heads", ptr(part), nsplit, C.byref(st), C.byref(sp), prefill, 0, ptr(dbg), stream)
            torch.cuda.synchronize()
            ref.append(tok.view(B, K).cpu())
            assert torch.equal(dbg_r[b].view(torch.int32), dbg[b].view(torch.int32)), (prefill, b)   # its CFG scale
        for b in range(B):
            assert (got[b] >= 0).all() and torch.equal(got[b], ref[b][b]), (prefill, b, got[b], ref[b][b])
            # the comparison can see a wrong row: row b under its neighbour's parameters samples other tokens
            assert not torch.equal(ref[(b + 1) % B][b], ref[b][b]), (prefill, b)
        if not prefill:                                       # the window bites: without the penalty row 3 differs
            tok = torch.full((B * K,), -1, **i32)
            d, _, cfg = HEADS_SETS[3]
            sp, st = _sp(d, cfg), state(HEADS_SEEDS[3], HEADS_KEYS[3] - 3, tok, torch.ones(B, device=DEV))
            call("zk_sample_heads", ptr(part), nsplit, C.byref(st), C.byref(sp), 0, 0, None, stream)
            torch.cuda.synchronize()
            free = tok.view(B, K).cpu()[3]
            assert (free[:, None] == hot).any(1).all(), (free, hot)
            assert not torch.equal(free, ref[3][3])


# ---------------------------------------------------------------------------- (b) a request in a batch == alone
def _tiny_engine(W):
    from zonos_amd.engine import EngineConfig, HipDecoder
    return HipDecoder(EngineConfig(TINY.d_model, TINY.n_layer, TINY.n_heads, TINY.n_kv, TINY.d_ff, TINY.eps), W, DEV)


def _utt(c, b):
    B = c["B"]
    return torch.stack([c["cond"][b], c["cond"][B + b]]), c["prefix"][b]


def mixed_requests(c, knobs_sp):
    """The three eos_sampled utterances as that fixture runs them (seed 1234, keys 0, 1, 2), one request with the
    sampled_knobs parameters, another seed and cfg_scale 3, and one greedy request with a budget of 5."""
    reqs = [Request(*_utt(c, b), c["max_new"], 2.0, c["sp"], c["seed"], b) for b in range(3)]
    reqs.append(Request(*_utt(c, 1), c["max_new"], 3.0, knobs_sp, 77, 5))
    reqs.append(Request(*_utt(c, 2), 5, 2.0, GREEDY, 3, 9))
    return reqs


def _alone(eng, r, **kw):
    """generate() of one request at B = 1: its arguments, row_base = its key."""
    return eng.generate(r.conditioning.to(DEV), r.audio_prefix_codes[None].to(DEV), r.max_new_tokens, r.cfg_scale, 1,
                        r.sampling_params, seed=r.seed, row_base=r.key, force_full_length=r.force_full_length,
                        **kw)[0].cpu()


@pytest.fixture(scope="module")
def mixed():
    c = load_gen_case("eos_sampled")
    reqs = mixed_requests(c, load_gen_case("sampled_knobs")["sp"])
    eng = _tiny_engine(c["W"])
    return dict(c=c, reqs=reqs, eng=eng, alone=[_alone(eng, r) for r in reqs])


@pytest.mark.parametrize("c_step", [True, False])
@pytest.mark.parametrize("use_graph", [True, False])
def test_request_in_batch_equals_request_alone(mixed, use_graph, c_step, monkeypatch):
    from zonos_amd.distributed import gemm_regime
    from zonos_amd.engine import ATTN_CHUNK, HipDecoder, attn_splits_for
    reqs, eng, alone = mixed["reqs"], mixed["eng"], mixed["alone"]
    lens = [int(a.shape[1]) for a in alone]
    budgets = [r.max_new_tokens for r in reqs]
    print("B = 1 lengths", lens, "budgets", budgets)
    # not vacuous, from the B = 1 runs themselves: two requests end by EOS at different steps, one of them while
    # another request is still running, and one runs out its budget
    by_eos = sorted(n for n, m in zip(lens, budgets) if n < m)
    assert len(set(by_eos)) >= 2, lens
    assert by_eos[0] < max(lens), lens
    assert any(n == m for n, m in zip(lens, budgets)), lens
    # one kernel regime: the batch and the B = 1 runs take the same GEMM path and attention split
    B, Lc, P = len(reqs), mixed["c"]["cond"].shape[1], mixed["c"]["prefix"].shape[2]
    assert B <= 8 and gemm_regime(B) == gemm_regime(1)
    smax = [-(-(Lc + P + n + 9) // ATTN_CHUNK) * ATTN_CHUNK for n in (max(budgets), min(budgets))]
    assert len({attn_splits_for(2 * b, TINY.n_kv, s) for b in (B, 1) for s in smax}) == 1
    monkeypatch.setattr(HipDecoder, "c_step", c_step)
    got = eng.generate_requests(reqs, use_graph=use_graph, poll_every=7)
    assert eng._ws["rows"] is not None and len(got) == B
    for b, (x, a) in enumerate(zip(got, alone)):
        assert x.shape == a.shape and torch.equal(x.cpu(), a), (b, x.shape, a.shape)
    # a generate() on the same engine afterwards is back on the batch-wide kernels
    assert torch.equal(_alone(eng, reqs[4]), alone[4]) and eng._ws["rows"] is None


# ---------------------------------------------------------------------------- (c) full width
# The 2-layer d_model 2048 geometry of the full-width engine tests (test_gpu_w8): B = 12 runs k_gemm_ws and the
# seven-launch sequence, B = 3 the five-launch GEMV sequence.
FULL_CFG = dict(d_model=2048, n_layer=2, n_heads=16, n_kv=4, d_ff=2048)
FULL_LC = 8
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


def _pool_request(i):
    from zonos_amd.synthetic import conditioning
    cond = conditioning(1, FULL_LC, FULL_CFG["d_model"], seed=100 + i)
    return Request(cond, None, 14 + (5 * i) % 11, (2.0, 3.0, 1.5)[i % 3], PARAM_POOL[i % 4], seed=1000 + 7 * i,
                   key=50 + 3 * i, force_full_length=i % 5 == 4)


@pytest.mark.parametrize("B,kw", [(12, {}), (3, {}), (12, dict(kv_dtype="fp8")), (3, dict(weight_dtype="fp8"))],
                         ids=["B12", "B3", "B12-kv8", "B3-w8"])
def test_neighbour_slot_and_regime_invariance_full_width(full_engine, B, kw):
    """The same requests among other neighbours and in other slots give the same codes: first + second run share
    half of their requests (six of twelve; two of three at B = 3), permuted."""
    pool = [_pool_request(i) for i in range(2 * B)]
    first = list(range(B))
    keep = first[::2] if B > 3 else [0, 2]                    # the common requests
    fresh = list(range(B, 2 * B))
    second = (keep[::-1] + fresh)[:B]
    second = second[1::2] + second[0::2]                      # interleave kept and new ones
    a = full_engine.generate_requests([pool[i] for i in first], poll_every=8, **kw)
    b = full_engine.generate_requests([pool[i] for i in second], poll_every=8, **kw)
    assert len(a) == len(b) == B
    assert all(x.shape[1] <= pool[i].max_new_tokens for i, x in zip(first, a))
    assert len({x.shape[1] for x in a}) > 1                   # rows end at different steps (their budgets)
    common = [i for i in keep if i in second]
    assert len(common) == (6 if B == 12 else 2)
    assert any(first.index(i) != second.index(i) for i in common)
    for i in common:
        x, y = a[first.index(i)], b[second.index(i)]
        assert x.shape == y.shape and torch.equal(x, y), (i, x.shape, y.shape)


# ---------------------------------------------------------------------------- (d) hybrid
def test_hybrid_requests_equal_requests_alone():
    from oracle import hybrid_ref as HR
    from zonos_amd.hybrid import HybridDecoder, HybridEngineConfig
    from zonos_amd.synthetic import conditioning
    h = HR.HybridCfg(d_model=256, n_layer=4, attn_layer_idx=(2,), n_heads=2, n_kv=1, d_ff=512, d_state=64, headdim=32)
    ec = HybridEngineConfig(d_model=h.d_model, n_layer=h.n_layer, attn_layer_idx=h.attn_layer_idx, n_heads=h.n_heads,
                            n_kv=h.n_kv, d_ff=h.d_ff, d_state=h.d_state, headdim=h.headdim, eps=h.eps, d_mlp=h.d_mlp,
                            rms_norm=h.rms_norm, residual_in_fp32=h.residual_in_fp32)
    eng = HybridDecoder(ec, HR.make_weights(h, seed=1), DEV)
    g = torch.Generator().manual_seed(5)
    reqs = []
    for i in range(3):
        cond = conditioning(1, 6, h.d_model, seed=20 + i)
        prefix = torch.randint(0, 1024, (9, 3), generator=g)
        reqs.append(Request(cond, prefix, (12, 7, 10)[i], (2.0, 3.0, 1.5)[i], PARAM_POOL[i], seed=5 + i, key=8 - i))
    got = eng.generate_requests(reqs, poll_every=5)
    for b, r in enumerate(reqs):
        a = _alone(eng, r)
        assert got[b].shape == a.shape and torch.equal(got[b].cpu(), a), (b, got[b].shape, a.shape)


# ---------------------------------------------------------------------------- (e) two ranks on the one GPU
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
        reqs = mixed_requests(c, load_gen_case("sampled_knobs")["sp"])
        eng = _tiny_engine(c["W"])
        local, allc = generate_sharded_requests(eng, reqs, coll_device="cpu", return_local=True, poll_every=5)
        one = eng.generate_requests(reqs, poll_every=5)
        ok = len(allc) == len(reqs) and all(x.shape == y.shape and torch.equal(x.cpu(), y.cpu())
                                            for x, y in zip(allc, one))
        q.put((rank, ok, len(local), [int(x.shape[1]) for x in allc], [int(x.shape[1]) for x in one]))
        dist.destroy_process_group()
    except Exception as e:       # report instead of hanging the parent
        q.put((rank, False, -1, repr(e), None))


def test_generate_sharded_requests_two_ranks():
    """Five requests with EOS enabled over two ranks (3 + 2, the short shard padded with a budget-less request):
    the gathered codes are one process's generate_requests."""
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
    assert len(set(res[0][3])) > 2, res                       # EOS at different steps, a spent budget


# ---------------------------------------------------------------------------- (f) uniform parameters
def test_uniform_requests_equal_generate_force_full_length():
    c = load_gen_case("sampled_knobs")
    eng = _tiny_engine(c["W"])
    B = c["B"]
    ref = eng.generate(c["cond"].to(DEV), c["prefix"].to(DEV), 16, 2.0, B, c["sp"], seed=11, force_full_length=True)
    ref = [x.clone() for x in ref]
    reqs = [Request(*_utt(c, b), 16, 2.0, c["sp"], 11, b, True) for b in range(B)]
    got = eng.generate_requests(reqs)
    assert all(x.shape == (9, 16) for x in ref)
    assert all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(got, ref))
