"""CPU: request batches (zonos_amd.requests, HipDecoder.generate_requests) -- the C ABI that carries the per-utterance
parameters (zk_row_params, the `rows` field of both step descriptors, the two _rows entries and their refusals), the
ValueErrors generate_requests raises before it touches a device, the per-request output trim, and
generate_sharded_requests over two gloo ranks."""
import ctypes as C
import os
import socket

import pytest
import torch

from oracle import zonos_ref
from zonos_amd.requests import EOS, MASK, Request, plan_requests, row_params, trim_request_codes


@pytest.fixture(scope="module")
def lib():
    from zonos_amd import build
    lib = C.CDLL(build.build())
    lib.zk_last_error.restype = C.c_char_p
    lib.zk_abi_size.restype = C.c_long
    lib.zk_abi_size.argtypes = [C.c_int]
    return lib


def test_abi_symbols_and_struct_mirrors(lib):
    from zonos_amd import _lib
    for name in ("zk_sample_heads_rows", "zk_eos_step_rows"):
        assert hasattr(lib, name) and name in _lib._SIGS and name in _lib.exported_symbols()
    R = _lib.RowParams
    assert lib.zk_abi_size(35) == C.sizeof(R) == C.sizeof(_lib.SamplingParams) + 16
    assert lib.zk_abi_size(36) == R.seed.offset == C.sizeof(_lib.SamplingParams) and R.sp.offset == 0
    assert lib.zk_abi_size(37) == R.key.offset == R.seed.offset + 8 and R.reserved.offset == R.key.offset + 4
    # rows is the last field of both descriptors ...
    for which, cls, prev in ((38, _lib.StepDesc, "w_fp8"), (39, _lib.HybridDesc, "xf")):
        assert cls._fields_[-1][0] == "rows" and cls._fields_[-2][0] == prev
        assert lib.zk_abi_size(which) == cls.rows.offset == C.sizeof(cls) - 8
    # ... and no earlier offset moved (the ids the earlier ABI tests pin)
    assert lib.zk_abi_size(7) == C.sizeof(_lib.StepDesc) and lib.zk_abi_size(19) == C.sizeof(_lib.HybridDesc)
    assert lib.zk_abi_size(1) == C.sizeof(_lib.GenState) and lib.zk_abi_size(0) == C.sizeof(_lib.SamplingParams)
    assert lib.zk_abi_size(13) == _lib.StepDesc.eps.offset and lib.zk_abi_size(14) == _lib.StepDesc.st.offset
    assert lib.zk_abi_size(15) == _lib.StepDesc.sp.offset and lib.zk_abi_size(24) == _lib.StepDesc.pre_k.offset
    assert lib.zk_abi_size(31) == _lib.StepDesc.w_fp8.offset == _lib.StepDesc.pre_smax.offset + 4
    assert _lib.StepDesc.rows.offset == _lib.StepDesc.w_fp8.offset + 4
    assert lib.zk_abi_size(20) == _lib.HybridDesc.st.offset and lib.zk_abi_size(21) == _lib.HybridDesc.eps.offset
    assert _lib.HybridDesc.rows.offset == _lib.HybridDesc.xf.offset + 8
    assert lib.zk_abi_size(40) == -1


def _buf():
    buf = C.create_string_buffer(256)
    return buf, C.cast(buf, C.c_void_p)


def test_step_entries_refuse_rows_with_torch_noise_without_gpu(lib):
    """rows together with st.noise_mode == 1 fails before any launch, in all four step entries."""
    from zonos_amd import _lib
    buf, p = _buf()
    lays = (_lib.StepLayer * 2)()
    d = _lib.StepDesc()
    d.B, d.n_layer, d.d_model, d.n_heads, d.n_kv, d.head_dim, d.smax = 1, 2, 2048, 16, 4, 128, 512
    d.layers = C.cast(lays, C.c_void_p)
    d.st.Ld, d.st.K, d.st.V, d.st.B = 100, 9, 1026, 1
    d.st.noise_mode, d.st.noise_stride, d.st.noise_incr = 1, 256, 4
    d.rows = p
    assert lib.zk_decode_step(C.byref(d), None) != 0
    err = lib.zk_last_error()
    assert b"zk_decode_step" in err and b"rows" in err and b"noise" in err, err
    lib.zk_prefill.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    assert lib.zk_prefill(C.byref(d), p, 4, 0, p, None) != 0
    err = lib.zk_last_error()
    assert b"zk_prefill" in err and b"rows" in err and b"noise" in err, err

    hl = (_lib.HybridLayer * 2)()
    h = _lib.HybridDesc()
    h.B, h.n_layer, h.d_model, h.n_heads, h.n_kv, h.head_dim, h.smax = 1, 2, 256, 2, 1, 128, 512
    h.d_inner, h.nheads_ssm, h.headdim_ssm, h.d_state = 512, 16, 32, 64
    h.layers = C.cast(hl, C.c_void_p)
    h.st.Ld, h.st.K, h.st.V, h.st.B = 100, 9, 1026, 1
    h.st.noise_mode, h.st.noise_stride, h.st.noise_incr = 1, 256, 4
    h.rows = p
    assert lib.zk_hybrid_decode_step(C.byref(h), None) != 0
    err = lib.zk_last_error()
    assert b"zk_hybrid_decode_step" in err and b"rows" in err and b"noise" in err, err
    lib.zk_hybrid_prefill.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    assert lib.zk_hybrid_prefill(C.byref(h), p, 4, 0, p, None) != 0
    err = lib.zk_last_error()
    assert b"zk_hybrid_prefill" in err and b"rows" in err and b"noise" in err, err


def test_rows_entries_refuse_without_gpu(lib):
    """zk_sample_heads_rows: NULL rows, torch noise, a NULL state / slab, a V the kernel cannot hold;
    zk_eos_step_rows: torch noise, a NULL state, too many codebooks. All before any launch."""
    from zonos_amd import _lib
    buf, p = _buf()
    lib.zk_sample_heads_rows.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                         C.c_void_p]
    lib.zk_eos_step_rows.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]

    def state(noise=0, V=1026, K=9):
        st = _lib.GenState()
        st.B, st.K, st.Ld, st.V = 2, K, 64, V
        st.noise_mode, st.noise_stride, st.noise_incr = noise, 256, 4
        return st

    st = state()
    assert lib.zk_sample_heads_rows(p, 1, C.byref(st), None, 0, 0, None, None) != 0
    err = lib.zk_last_error()
    assert b"zk_sample_heads_rows" in err and b"null rows" in err, err
    st = state(noise=1)
    assert lib.zk_sample_heads_rows(p, 1, C.byref(st), p, 0, 0, None, None) != 0
    err = lib.zk_last_error()
    assert b"zk_sample_heads_rows" in err and b"noise" in err, err
    assert lib.zk_sample_heads_rows(p, 1, None, p, 0, 0, None, None) != 0 and b"null" in lib.zk_last_error()
    st = state()
    assert lib.zk_sample_heads_rows(None, 1, C.byref(st), p, 0, 0, None, None) != 0 and b"null" in lib.zk_last_error()
    st = state(V=1281)
    assert lib.zk_sample_heads_rows(p, 1, C.byref(st), p, 0, 0, None, None) != 0 and b"V=1281" in lib.zk_last_error()

    st = state(noise=1)
    assert lib.zk_eos_step_rows(C.byref(st), 0, 0, None) != 0
    err = lib.zk_last_error()
    assert b"zk_eos_step_rows" in err and b"noise" in err, err
    assert lib.zk_eos_step_rows(None, 0, 0, None) != 0 and b"zk_eos_step_rows" in lib.zk_last_error()
    st = state(K=17)
    assert lib.zk_eos_step_rows(C.byref(st), 0, 0, None) != 0 and b"K=17" in lib.zk_last_error()


# ---------------------------------------------------------------------------- generate_requests' refusals
D = 2048


def _req(Lc=4, P=0, **kw):
    prefix = torch.zeros(9, P, dtype=torch.int64) if P else None
    return Request(torch.zeros(2, Lc, D, dtype=torch.bfloat16), prefix, **kw)


def _bare(cls):
    from zonos_amd.engine import EngineConfig
    eng = cls.__new__(cls)                          # no weights, no device: the refusals come before both
    eng.cfg = EngineConfig(d_model=D, n_layer=2, n_heads=16, n_kv=4, d_ff=2048)
    eng.rope_neox = 0
    eng._ws = None
    return eng


@pytest.mark.parametrize("engine", ["HipDecoder", "HybridDecoder"])
def test_generate_requests_refusals_need_no_device(engine):
    from zonos_amd.engine import HipDecoder
    from zonos_amd.hybrid import HybridDecoder
    eng = _bare(dict(HipDecoder=HipDecoder, HybridDecoder=HybridDecoder)[engine])
    with pytest.raises(ValueError, match="empty"):
        eng.generate_requests([])
    with pytest.raises(ValueError, match="ragged prompts are not supported"):
        eng.generate_requests([_req(Lc=4), _req(Lc=5)])
    with pytest.raises(ValueError, match="ragged prompts are not supported"):
        eng.generate_requests([_req(P=2), _req(P=3)])
    with pytest.raises(ValueError, match="ragged prompts are not supported"):
        eng.generate_requests([_req(P=2), _req(P=0)])
    with pytest.raises(ValueError, match="request 1: cfg_scale == 1"):
        eng.generate_requests([_req(), _req(cfg_scale=1.0)])
    for w in (0, 513, -1):
        with pytest.raises(ValueError, match="request 1: repetition_penalty_window"):
            eng.generate_requests([_req(), _req(sampling_params=dict(repetition_penalty_window=w))])
    with pytest.raises(ValueError, match="conditioning must be"):
        eng.generate_requests([Request(torch.zeros(4, 4, D))])
    with pytest.raises(ValueError, match="max_new_tokens"):
        eng.generate_requests([_req(max_new_tokens=0)])
    assert eng._ws is None


def test_plan_and_row_params():
    """The per-request state the engine uploads: merged parameters, budgets, [cond | uncond] stacking."""
    from zonos_amd import _lib
    from zonos_amd.requests import DEFAULT_SAMPLING, budget_mask, stack_conditioning, stack_prefixes
    a = Request(torch.full((2, 3, 8), 1.0), torch.full((1, 9, 2), 5), 7, 3.0, dict(top_k=4, temperature=0.5), 11, 40, True)
    b = Request(torch.full((2, 3, 8), 2.0), torch.full((9, 2), 6), 3)
    b.conditioning[1] = 20.0
    a.conditioning[1] = 10.0
    plan = plan_requests([a, b], 8, pad=1)
    assert (plan.Lc, plan.P, plan.budgets, plan.max_new, plan.real) == (3, 2, [7, 0], 7, 1)
    assert plan.params[0]["top_k"] == 4 and plan.params[0]["linear"] == DEFAULT_SAMPLING["linear"]
    assert plan.params[1] == DEFAULT_SAMPLING
    rows = row_params(plan_requests([a, b], 8))
    assert C.sizeof(rows) == 2 * C.sizeof(_lib.RowParams)
    assert (rows[0].sp.top_k, rows[0].sp.temperature, rows[0].sp.cfg_scale, rows[0].sp.force_full_length,
            rows[0].seed, rows[0].key, rows[0].reserved) == (4, 0.5, 3.0, 1, 11, 40, 0)
    assert (rows[1].sp.top_k, rows[1].sp.rp_window, rows[1].sp.cfg_scale, rows[1].sp.force_full_length, rows[1].seed,
            rows[1].key) == (0, 2, 2.0, 0, 0, 0)
    cond = stack_conditioning(plan)
    assert cond.shape == (4, 3, 8) and cond[:, 0, 0].tolist() == [1.0, 2.0, 10.0, 20.0]
    pre = stack_prefixes(plan)
    assert pre.shape == (2, 9, 2) and pre[:, 0, 0].tolist() == [5, 6]
    assert stack_prefixes(plan_requests([Request(torch.zeros(2, 3, 8))], 8)) is None
    # frames past a request's budget hold MASK before the delay pattern; the prefix and its frames stay
    codes = torch.full((2, 9, 9), -1)
    codes[..., :2] = pre
    budget_mask(codes, 2, [7, 3])
    assert (codes[0] == -1)[:, 2:].all() and (codes[1, :, 2:5] == -1).all() and (codes[1, :, 5:] == MASK).all()
    assert torch.equal(codes[..., :2], pre)


# ---------------------------------------------------------------------------- the output trim
def _delayed(codes):
    return zonos_ref.apply_delay(codes)


def test_trim_request_codes():
    """Hand-built final delayed codes, P = 2, Ld sized for the largest budget (10)."""
    P, Tmax = 2, 12
    g = torch.Generator().manual_seed(0)
    codes = torch.randint(0, 1024, (6, 9, Tmax), generator=g)
    want = codes.clone()
    budgets = [10, 6, 6, 1, 5, 10]
    # row 0: ended by EOS at new frame 4, before its budget; the staircase and MASKs behind it
    codes[0, 0, P + 4] = EOS
    codes[0, 1:, P + 4:] = MASK
    codes[0, 0, P + 5:] = MASK
    # row 1: ended by its budget; an in-range MASK / EOS of a higher codebook is zeroed, not a stop
    codes[1, 3, P + 2] = MASK
    codes[1, 5, P + 3] = EOS
    want[1, 3, P + 2] = want[1, 5, P + 3] = 0
    # row 2: wrote EOS / MASK after its budget (frames >= P + 6): must not shorten or alter it
    codes[2, 0, P + 6] = EOS
    codes[2, 0, P + 7:] = MASK
    codes[2, 1:, P + 6:] = MASK
    # row 3: n = 1; row 4: n < 9 with an EOS exactly at its budget's end (not inside it)
    codes[4, 0, P + 5] = EOS
    # row 5: EOS at the first new frame -> an empty result
    codes[5, 0, P] = EOS
    out = trim_request_codes(_delayed(codes), P, budgets)
    assert [o.shape[1] for o in out] == [4, 6, 6, 1, 5, 0]
    for b, o in enumerate(out):
        assert o.dtype == torch.int64 and o.shape[0] == 9 and torch.equal(o, want[b, :, P:P + o.shape[1]]), b
        assert (o < 1024).all()
    # an early-ended loop (callback): only the frames final at `offset` (t < offset - 9)
    cut = trim_request_codes(_delayed(codes), P, budgets, offset=P + 3 + 9)
    assert [o.shape[1] for o in cut] == [3, 3, 3, 1, 3, 0]
    # equals the single-request trim of the reference restatement for every row (its own Ld, its own offset)
    for b, n in enumerate(budgets):
        alone = _delayed(codes[b:b + 1, :, :P + n])
        ref = zonos_ref.revert_delay(alone)[0, :, :P + n]
        eos = (ref[0] == EOS).nonzero()
        end = int(eos[0]) if eos.numel() and int(eos[0]) > 0 else P + n
        ref = ref[:, P:end].clone()
        ref[ref >= 1024] = 0
        assert torch.equal(out[b], ref), b


# ---------------------------------------------------------------------------- sharding (gloo, world 2)
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class StubRequestEngine:
    """Stands in for HipDecoder.generate_requests: a request's codes are a function of the request alone."""

    def __init__(self):
        self.calls = []

    @staticmethod
    def codes_of(r):
        v = (int(r.conditioning[0, 0, 0]) * 31 + int(r.conditioning[1, 0, 0]) + r.seed * 7 + r.key) % 1024
        return torch.full((9, 1 + r.max_new_tokens % 4), v, dtype=torch.int64)

    def generate_requests(self, requests, *, _pad=0, **kw):
        reqs = list(requests)
        self.calls.append(([int(r.conditioning[0, 0, 0]) for r in reqs], _pad, sorted(kw)))
        return [self.codes_of(r) for r in reqs[:len(reqs) - _pad]]


def _requests(B):
    out = []
    for i in range(B):
        c = torch.zeros(2, 3, 4)
        c[0, 0, 0], c[1, 0, 0] = i, 100 + i
        out.append(Request(c, None, max_new_tokens=5 + i, seed=3 * i, key=B - i))
    return out


def _sharded_worker(rank, world, port, q):
    import torch.distributed as dist
    from zonos_amd.distributed import generate_sharded_requests
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    reqs = _requests(5)
    ref = [StubRequestEngine.codes_of(r) for r in reqs]
    eng = StubRequestEngine()
    got = generate_sharded_requests(eng, reqs, coll_device="cpu", kv_dtype="fp8")
    ok = len(got) == 5 and all(torch.equal(a, b) for a, b in zip(got, ref))
    eng2 = StubRequestEngine()
    mine, allc = generate_sharded_requests(eng2, reqs, coll_device="cpu", uniform_shards=False, return_local=True)
    ok = ok and len(allc) == 5 and all(torch.equal(a, b) for a, b in zip(allc, ref))
    q.put((rank, ok, eng.calls, eng2.calls, len(mine)))
    dist.destroy_process_group()


def test_generate_sharded_requests_gloo_world2():
    """B = 5 over 2 ranks: contiguous slices 3 + 2; the short shard is padded with one budget-less request
    (_pad = 1) whose codes are dropped; the gathered list is the per-request codes in request order."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_sharded_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = sorted(q.get(timeout=120) for _ in ps)
    for p in ps:
        p.join(timeout=60)
    assert all(r[1] for r in res), res
    assert res[0][2] == [([0, 1, 2], 0, ["kv_dtype"])] and res[1][2] == [([3, 4, 4], 1, ["kv_dtype"])], res
    assert res[0][3] == [([0, 1, 2], 0, [])] and res[1][3] == [([3, 4], 0, [])], res
    assert [r[4] for r in res] == [3, 2]


def test_generate_sharded_requests_single_process():
    from zonos_amd.distributed import generate_sharded_requests
    reqs = _requests(4)
    eng = StubRequestEngine()
    got = generate_sharded_requests(eng, reqs)
    assert all(torch.equal(a, StubRequestEngine.codes_of(r)) for a, r in zip(got, reqs)) and eng.calls[0][1] == 0
    with pytest.raises(ValueError, match="empty"):
        generate_sharded_requests(eng, [])


def test_request_is_reexported():
    import zonos.model as ref_surface
    import zonos_amd.model as zm
    assert zm.Request is Request and ref_surface.Request is Request
    assert hasattr(zm.Zonos, "generate_requests")
