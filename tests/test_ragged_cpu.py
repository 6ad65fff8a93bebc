"""CPU: ragged request batches (generate_requests(ragged=True)) -- the plan, the padded stack, the refusals that need
no device and the C ABI of the per-row-context entries.

The offsets travel as an argument of zk_prefill_rows / zk_decode_step_rows, not as a field of zk_step_desc:
tests/test_requests_cpu.py pins `rows` as the descriptor's last field, its size and `zk_abi_size(40) == -1`, so
the descriptor cannot grow. What is checked here in its place: the two entries and the four kernel entries are
exported, declared and bound, the descriptor kept its layout, and zk_version() >= 3."""
import ctypes as C

import pytest
import torch

from zonos_amd.requests import Request, plan_requests, stack_conditioning

D = 2048


def _req(Lc=4, P=2, **kw):
    g = torch.Generator().manual_seed(Lc * 10 + P)
    return Request(torch.randn(2, Lc, D, generator=g).to(torch.bfloat16),
                   torch.randint(0, 1024, (9, P), generator=g) if P else None, **kw)


def test_plan_ragged_lengths_and_padded_stack():
    reqs = [_req(4), _req(7), _req(5)]
    plan = plan_requests(reqs, D, ragged=True)
    assert plan.Lc == 7 and plan.lcs == [4, 7, 5] and plan.P == 2
    assert plan.row_off == [-3, 0, -2, -3, 0, -2]
    x = stack_conditioning(plan)
    assert x.shape == (6, 7, D)
    for b, r in enumerate(reqs):
        n = r.conditioning.shape[1]
        for half in (0, 1):                                   # cond rows, then uncond rows
            row = x[half * 3 + b]
            assert torch.equal(row[:n], r.conditioning[half]) and not row[n:].any()
    # the engine's test hook: another finite value in the padding, the tokens untouched
    y = stack_conditioning(plan, 1e4)
    assert torch.equal(y[0, :4], x[0, :4]) and (y[0, 4:] == torch.tensor(1e4, dtype=torch.bfloat16)).all()
    assert torch.equal(y[1], x[1])


def test_equal_lengths_take_the_uniform_path():
    plan = plan_requests([_req(6), _req(6)], D, ragged=True)
    assert plan.row_off is None and plan.Lc == 6 and plan.lcs == [6, 6]
    assert stack_conditioning(plan).shape == (4, 6, D)
    assert plan_requests([_req(6), _req(6)], D).row_off is None


def test_default_and_ragged_prefix_refusals():
    with pytest.raises(ValueError, match="^ragged prompts are not supported"):
        plan_requests([_req(4), _req(5)], D)
    with pytest.raises(ValueError, match="^ragged prompts are not supported"):
        plan_requests([_req(4), _req(5)], D, ragged=False)
    # audio prefixes of different lengths stay refused
    for a, b in ((2, 3), (2, 0)):
        with pytest.raises(ValueError, match="^ragged prompts are not supported"):
            plan_requests([_req(4, a), _req(5, b)], D, ragged=True)
        with pytest.raises(ValueError, match="^ragged prompts are not supported"):
            plan_requests([_req(4, a), _req(4, b)], D, ragged=True)
    with pytest.raises(ValueError, match="at least one token"):
        plan_requests([_req(0), _req(5)], D, ragged=True)


def _bare(cls):
    from zonos_amd.engine import EngineConfig
    eng = cls.__new__(cls)                          # no weights, no device: the refusals come before both
    eng.cfg = EngineConfig(d_model=D, n_layer=2, n_heads=16, n_kv=4, d_ff=2048)
    eng.rope_neox = 0
    eng._ws = None
    return eng


def test_hybrid_engine_refuses_differing_lengths_before_any_allocation():
    from zonos_amd.engine import HipDecoder
    from zonos_amd.hybrid import HybridDecoder
    eng = _bare(HybridDecoder)
    with pytest.raises(ValueError, match="ragged=True with conditionings of different lengths"):
        eng.generate_requests([_req(4), _req(5)], ragged=True)
    assert eng._ws is None
    with pytest.raises(ValueError, match="^ragged prompts are not supported"):
        eng.generate_requests([_req(4), _req(5)])
    # the transformer engine with GPT-NeoX RoPE (no such model ships; the rows kernels are interleaved only)
    eng = _bare(HipDecoder)
    eng.rope_neox = 1
    with pytest.raises(ValueError, match="interleaved RoPE"):
        eng.generate_requests([_req(4), _req(5)], ragged=True)
    assert eng._ws is None


@pytest.fixture(scope="module")
def lib():
    from zonos_amd import build
    lib = C.CDLL(build.build())
    lib.zk_last_error.restype = C.c_char_p
    lib.zk_abi_size.restype = C.c_long
    lib.zk_abi_size.argtypes = [C.c_int]
    return lib


ENTRIES = ("zk_attn_decode_qkv_sc_rows", "zk_attn_decode_qkv_f8_rows", "zk_embed_codes_rows", "zk_gather_last_rows",
           "zk_prefill_rows", "zk_decode_step_rows")


def test_abi_version_entries_and_descriptor(lib):
    from zonos_amd import _lib
    lib.zk_version.restype = C.c_int
    assert lib.zk_version() >= 3
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _lib._SIGS and name in _lib.exported_symbols(), name
    # one more pointer than the uniform entry each, the descriptor as it was
    for rows, plain in (("zk_attn_decode_qkv_sc_rows", "zk_attn_decode_qkv_sc"),
                        ("zk_attn_decode_qkv_f8_rows", "zk_attn_decode_qkv_f8"), ("zk_prefill_rows", "zk_prefill"),
                        ("zk_decode_step_rows", "zk_decode_step")):
        extra = 0 if rows != "zk_attn_decode_qkv_sc_rows" else 1          # (_sc_rows has no rope_neox argument)
        assert len(_lib._SIGS[rows]) == len(_lib._SIGS[plain]) + 1 - extra, rows
    assert lib.zk_abi_size(7) == C.sizeof(_lib.StepDesc) and lib.zk_abi_size(38) == _lib.StepDesc.rows.offset


def test_rows_entries_refuse_bad_arguments_without_gpu(lib):
    """Every check of the rows forms comes before the launch, with the entry's own name in the message."""
    buf = C.create_string_buffer(256)
    p = C.cast(buf, C.c_void_p)
    V, I, F = C.c_void_p, C.c_int, C.c_float
    fn = lib.zk_attn_decode_qkv_sc_rows
    fn.argtypes = [V, I, V, V, V, I, I, I, I, I, I, V, V, V, I, V, V, V, V]
    # NULL row_off, then hd != 128
    assert fn(p, 1, p, p, p, 2, 8, 2, 128, 256, 1, p, None, p, 1, None, p, None, None) != 0
    assert b"zk_attn_decode_qkv_sc_rows" in lib.zk_last_error() and b"row_off" in lib.zk_last_error()
    assert fn(p, 1, p, p, p, 2, 8, 2, 64, 256, 1, p, p, p, 1, None, p, None, None) != 0
    assert lib.zk_last_error().startswith(b"zk_attn_decode_qkv_sc_rows: head_dim")
    f8 = lib.zk_attn_decode_qkv_f8_rows
    f8.argtypes = [V, I, V, V, V, V, V, I, I, I, I, I, I, V, V, V, I, V, V, V, V]
    assert f8(p, 1, p, p, p, p, p, 2, 8, 2, 128, 256, 1, p, None, p, 1, None, p, None, None) != 0
    assert b"zk_attn_decode_qkv_f8_rows" in lib.zk_last_error() and b"row_off" in lib.zk_last_error()
    emb = lib.zk_embed_codes_rows
    emb.argtypes = [V, I, I, I, C.c_long, C.c_long, V, I, I, I, V, I, I, V, V]
    assert emb(p, 1, 3, 9, 9, 1, p, 1026, 256, 2, p, 8, 4, None, None) != 0
    assert lib.zk_last_error().startswith(b"zk_embed_codes_rows: NULL")
    assert emb(p, 1, 3, 9, 9, 1, p, 1026, 256, 2, p, 2, 0, p, None) != 0       # out_S < S
    assert lib.zk_last_error().startswith(b"zk_embed_codes_rows: out_S")
    ga = lib.zk_gather_last_rows
    ga.argtypes = [V, I, I, I, V, V, V]
    assert ga(p, 2, 4, 256, None, p, None) != 0 and lib.zk_last_error().startswith(b"zk_gather_last_rows: NULL")
    # the step entries: attn_merge > 0 and rope_neox are refused with row_off before anything is enqueued
    from zonos_amd import _lib
    layers = (_lib.StepLayer * 1)()
    for field, msg in (("attn_merge", b"attn_merge = 4"), ("rope_neox", b"rope_neox = 1")):
        d = _lib.StepDesc()
        d.B, d.n_layer, d.layers = 2, 1, C.cast(layers, C.c_void_p)
        setattr(d, field, 4 if field == "attn_merge" else 1)
        for name, args in (("zk_decode_step_rows", (C.byref(d), p, None)),
                           ("zk_prefill_rows", (C.byref(d), p, 4, 0, p, p, None))):
            f = getattr(lib, name)
            f.argtypes = [V, V, V] if name == "zk_decode_step_rows" else [V, V, I, I, V, V, V]
            assert f(*args) != 0
            err = lib.zk_last_error()
            assert err.startswith(name.encode() + b": row_off") and msg in err, err
