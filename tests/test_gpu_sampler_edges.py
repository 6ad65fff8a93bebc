"""GPU: the three sampler entries against the fp64 reference on rows in which one wrongly kept or dropped
token, one history column or one count changes the winner (tests/sampler_probe.py). Acceptance is zero flipped
tokens on the rows the probe selected (race margin >= 1 + 2^-7, decision margin >= 2^-10; the fp32 oracle's
measured deviation is below an eighth of either, tests/test_sampler_probe_cpu.py). Also the window contract of
include/zonos_hip.h: the windows that fit against the reference, the others through the entries' refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

from zonos_amd import _lib
from zonos_amd import sampling as zs
from zonos_amd._lib import GenState, SamplingParams, ptr

from . import sampler_probe as sp

pytestmark = pytest.mark.gpu
DEV = "cuda"
POISON = -7


@pytest.fixture(scope="module", autouse=True)
def _load():
    _lib.load()


@pytest.fixture(scope="module")
def fam():
    return sp.families()


def _params(kw, cfg_scale=1.0, ffl=0):
    return SamplingParams(float(kw.get("temperature", 1.0)), float(kw.get("top_p", 0)), float(kw.get("min_p", 0)),
                          float(kw.get("linear", 0)), float(kw.get("conf", 0)), float(kw.get("quad", 0)),
                          int(kw.get("top_k", 0)), int(kw.get("repetition_penalty_window", 2)), cfg_scale, ffl)


def _rc(name, *args):
    """(return code, message) of a C entry that may refuse."""
    lib = _lib.load()
    rc = getattr(lib, name)(*args)
    return rc, lib.zk_last_error().decode()


def _sample_direct(case):
    """The entry itself: gen_stride and gen_len as the case has them."""
    B, K, V = case.shape
    lg = torch.from_numpy(case.logits).to(DEV)
    gen = None if case.gen is None else torch.from_numpy(case.gen).to(DEV)
    rp = torch.from_numpy(case.rp).to(DEV)
    out = torch.full((B, K), POISON, dtype=torch.int64, device=DEV)
    co = case.coords
    par = _params(case.sp)
    rc, msg = _rc("zk_sample_logits", ptr(lg), B, K, V, ptr(gen), 0 if gen is None else gen.shape[2], case.gen_len,
                  ptr(rp), C.byref(par), co["seed"], co["step"], co["draw"], co["row_base"], ptr(out),
                  _lib.stream_ptr(lg.device))
    torch.cuda.synchronize()
    return rc, msg, out.cpu().numpy()


def _sample(case, **stream):
    """sample_from_logits on one case (the C entry where the case needs its own gen_stride)."""
    if case.direct:
        rc, msg, tok = _sample_direct(case)
        assert rc == 0, msg
        return tok
    kw = dict(case.sp)
    if case.gen is not None:
        kw.update(generated_tokens=torch.from_numpy(case.gen[..., :case.gen_len]).to(DEV),
                  repetition_penalty=torch.from_numpy(case.rp))
    return zs.sample_from_logits(torch.from_numpy(case.logits).to(DEV), **kw, **stream).squeeze(-1).cpu().numpy()


def _flips(case, tok):
    bad = (tok != case.tok) & case.use
    return [(case.name, b, k, int(tok[b, k]), int(case.tok[b, k]), int(case.decisive[b, k]), int(case.variant[b, k]))
            for b, k in zip(*np.nonzero(bad))]


# ---------------------------------------------------------------------------- zk_sample_logits, keyed stream
@pytest.mark.parametrize("family", ["top_k", "top_p", "min_p", "unified_min_p", "all_filters", "greedy_rp"])
def test_keyed_stream(fam, family):
    flips, rows = [], 0
    for c in fam[family]:
        assert c.shape[0] * c.shape[1] <= 72
        flips += _flips(c, _sample(c, **c.coords))
        rows += int(c.use.sum())
    print(f"zk_sample_logits {family}: {len(flips)} flips of {rows} rows in {len(fam[family])} calls")
    assert not flips, flips[:8]


# ---------------------------------------------------------------------------- zk_sample_logits_torch
def test_torch_stream():
    """The rows are built here from torch's own stream at the stride the device's policy gives; afterwards the
    generator stands where torch's own exponential_ calls leave it."""
    seed = 20240607
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    g2 = torch.Generator(device=DEV)
    g2.manual_seed(seed)
    cases = sp.torch_ladder_cases(lambda n: zs.torch_noise_policy(n, DEV), seed, int(g.get_offset()))
    flips, rows = [], 0
    for c, off, stride, incr in cases:
        assert int(g.get_offset()) == off
        flips += _flips(c, _sample(c, generator=g))
        rows += int(c.use.sum())
        torch.empty(c.shape, device=DEV).exponential_(1, generator=g2)
        assert int(g.get_offset()) == int(g2.get_offset()) == off + incr
    share = sp.left_out([c for c, *_ in cases])
    print(f"zk_sample_logits_torch: {len(flips)} flips of {rows} rows in {len(cases)} calls, "
          f"{share * 100:.2f} % left out")
    assert share <= sp.MAX_LEFT_OUT
    assert not flips, flips[:8]
    assert torch.equal(g.get_state(), g2.get_state())


# ---------------------------------------------------------------------------- greedy ties
def test_greedy_ties_return_the_lowest_index():
    """temperature 0 with exact ties: torch.argmax's first index. Ties across two waves (63 | 64), across
    register slots (255 | 256, 1023 | 1024), within one lane's slots (100, 356, 612, 868) and everywhere."""
    ties = [(63, 64), (255, 256), (1023, 1024), (1024, 1025), (0, 1025), (127, 128, 129), (100, 356, 612, 868),
            (191, 192), (300, 1025), (5, 1024), (256, 512, 768, 1024), tuple(range(1026))]
    B, K, V = 2, 6, 1026
    logits = torch.randn(B, K, V, generator=torch.Generator().manual_seed(5)).clamp(max=3.0)
    for i, t in enumerate(ties):
        logits[i // K, i % K, list(t)] = 4.0
    tok = zs.sample_from_logits(logits.to(DEV), temperature=0.0, seed=3).reshape(-1).cpu().tolist()
    assert tok == [min(t) for t in ties]


# ---------------------------------------------------------------------------- zk_sample_heads
class Heads:
    """A zk_gen_state over small device buffers, driven directly."""

    def __init__(self, B, K, V, Ld, seed=0, row_base=0):
        i32 = dict(dtype=torch.int32, device=DEV)
        self.B, self.K, self.V = B, K, V
        self.scal = torch.zeros(16, **i32)
        self.eos_mode, self.steps_after, self.remaining, self.stopping, self.act = (torch.zeros(B, **i32)
                                                                                  for _ in range(5))
        self.rp = torch.ones(B, dtype=torch.float32, device=DEV)
        self.tok0 = torch.full((B * K,), POISON, **i32)
        self.tok1 = torch.full((B * K,), POISON, **i32)
        self.delayed = torch.full((B, K, Ld), 7, dtype=torch.int64, device=DEV)
        self.st = GenState(ptr(self.scal), ptr(self.eos_mode), ptr(self.steps_after), ptr(self.remaining),
                           ptr(self.stopping), ptr(self.act), ptr(self.rp), ptr(self.tok0), ptr(self.tok1),
                           ptr(self.delayed), B, K, Ld, V, seed & 0xFFFFFFFFFFFFFFFF, row_base, 0, 0, 0, 0)

    def set_scal(self, offset=0, step=0, done=0, nres=0):
        self.scal.copy_(torch.tensor([offset, 0, step, done, nres] + [0] * 11, dtype=torch.int32))

    def run(self, slabs, kw, prefill=0, draw=0, ffl=0):
        part = torch.from_numpy(slabs).to(DEV)
        par = _params(kw, cfg_scale=2.0, ffl=ffl)
        rc, msg = _rc("zk_sample_heads", ptr(part), slabs.shape[0], C.byref(self.st), C.byref(par), prefill, draw,
                      None, _lib.stream_ptr(part.device))
        torch.cuda.synchronize()
        return rc, msg

    def tokens(self, draw=0):
        return (self.tok1 if draw else self.tok0).view(self.B, self.K).cpu().numpy().astype(np.int64)


def _with_mask_bait(combined, value):
    """Token 1025 gets the row's largest logit in the slabs: it never wins (model.py:115)."""
    x = combined.copy()
    x[..., sp.MASK] = value
    return x


@pytest.mark.parametrize("nsplit", [1, 2, 3])
def test_heads_top_k(nsplit):
    """The top-k rows through the CFG combine of nsplit slabs: history-free (rp = 1), step / draw / row_base
    of the keyed stream from the state."""
    B, K, V = sp.B_DEF, sp.K_DEF, 1026
    rng = np.random.default_rng(nsplit)
    flips, rows, cases = [], 0, []
    for k, (step, row_base) in zip((1, 2, 20, 20), ((1, 0), (17, 3), (3005, 16), (260, 7))):
        co = dict(seed=sp.KEYED_SEED + 77 + nsplit, step=step, draw=0, row_base=row_base)
        noise = sp.keyed_noise(co, B, K, V)
        base = sp.ladder_case("heads_top_k", f"k{k}-s{step}", noise, co, nkept=k, d=0.0625, sp=dict(top_k=k),
                              plateau=40, forbid=sp.HEADS_FORBID, seed=nsplit)
        combined = _with_mask_bait(base.logits, 8.0)
        case = sp.Case(base.family, base.name, base.sp, sp.heads_logits(combined), noise, base.variant,
                       base.decisive, co).finish()
        h = Heads(B, K, V, Ld=8, seed=co["seed"], row_base=row_base)
        h.set_scal(offset=4, step=step)
        rc, msg = h.run(sp.heads_slabs(combined, nsplit, 2.0, rng), case.sp)
        assert rc == 0, msg
        tok = h.tokens()
        assert not (tok == sp.MASK).any()
        assert (h.tok1 == POISON).all()
        flips += _flips(case, tok)
        rows += int(case.use.sum())
        cases.append(case)
    share = sp.left_out(cases)
    print(f"zk_sample_heads top_k nsplit {nsplit}: {len(flips)} flips of {rows} rows, {share * 100:.2f} % left out")
    assert share <= sp.MAX_LEFT_OUT
    assert not flips, flips[:8]


def _heads_greedy(nsplit, window, gen_len, Ld, seed):
    base = sp.greedy_case(f"heads-W{window}-len{gen_len}", 1026, window, gen_len, Ld, sp.RPS, (8.0, -2.0, 4.0, 0.0),
                          quantum=0.25, seed=seed, forbid=sp.HEADS_FORBID)
    combined = _with_mask_bait(base.logits, 16.0)
    case = sp.Case(base.family, base.name, base.sp, sp.heads_logits(combined), None, base.variant, base.decisive,
                   base.coords, base.gen, gen_len, base.rp, tags=base.tags).finish()
    return case, combined


@pytest.mark.parametrize("nsplit,window,gen_len", [(1, 8, 19), (2, 8, 5), (3, 512, 600), (1, 1, 3)])
def test_heads_greedy_repetition_penalty(nsplit, window, gen_len):
    """History in st.delayed, its length in scal[0], rp per row in st.rp."""
    Ld = gen_len + 5
    case, combined = _heads_greedy(nsplit, window, gen_len, Ld, seed=40 + nsplit)
    B, K, V = case.shape
    h = Heads(B, K, V, Ld)
    h.delayed.copy_(torch.from_numpy(case.gen))
    h.rp.copy_(torch.from_numpy(case.rp))
    h.set_scal(offset=gen_len, step=3)
    rc, msg = h.run(sp.heads_slabs(combined, nsplit, 2.0, np.random.default_rng(nsplit)), case.sp)
    assert rc == 0, msg
    flips = _flips(case, h.tokens())
    print(f"zk_sample_heads greedy W{window} len{gen_len} nsplit {nsplit}: {len(flips)} flips of "
          f"{int(case.use.sum())} rows, {sp.left_out([case]) * 100:.2f} % left out")
    assert sp.left_out([case]) <= sp.MAX_LEFT_OUT
    assert not flips, flips[:8]
    # prefill: no penalty (and no history read)
    ref = sp.reference(sp.heads_logits(combined, prefill=True), None, case.sp)[0]
    h.tok0.fill_(POISON)
    rc, msg = h.run(sp.heads_slabs(combined, nsplit, 2.0, np.random.default_rng(9)), case.sp, prefill=1)
    assert rc == 0, msg
    assert np.array_equal(h.tokens(), ref)


def _eos_rows(B, K, V, rng):
    """Greedy rows whose only candidates are EOS (logit 10 in the slabs) and token 7. Row b's token-7 logit:
    3.0625 -> EOS - log 1024 = 3.0685 wins by 0.2 %; 3.09375 -> EOS loses by 0.8 % (the nearest values on either
    side that the bf16 slabs hold exactly and that keep the 2^-10 decision margin: a bias constant wrong by
    0.2 % of the logit changes a winner); 0 -> EOS wins outright wherever a rule does not forbid it. Token 1025
    holds the largest logit of all."""
    combined = (-96.0 - 4.0 * rng.integers(0, 7, size=(B, K, V))).astype(np.float32)
    combined[..., sp.EOS] = 10.0
    combined[..., 7] = np.array([3.0625, 3.09375, 0.0, 0.0, 3.0625, 3.09375, 0.0, 0.0], dtype=np.float32)[:B, None]
    return _with_mask_bait(combined, 16.0)


@pytest.mark.parametrize("nsplit", [1, 3])
def test_heads_eos_column(nsplit):
    B, K, V = 8, sp.K_DEF, 1026
    rng = np.random.default_rng(100 + nsplit)
    combined = _eos_rows(B, K, V, rng)
    slabs = sp.heads_slabs(combined, nsplit, 2.0, rng)
    kw = dict(temperature=0.0, repetition_penalty_window=2)

    def expect(**rules):
        x = sp.heads_logits(combined, **rules)
        tok, _, dec = sp.reference(x, None, kw)
        assert (dec >= sp.DECISION_MARGIN).all()
        return tok

    # (the biased rows decide by little more than the decision margin: within a factor 10 of it)
    dec0 = sp.reference(sp.heads_logits(combined), None, kw)[2][[0, 1, 4, 5], 0]
    assert (dec0 >= sp.DECISION_MARGIN).all() and (dec0 <= 10 * sp.DECISION_MARGIN).all(), dec0

    h = Heads(B, K, V, Ld=8)
    h.set_scal(offset=4, step=2)
    # the bias decides by the decision margin on codebook 0; codebooks >= 1 never take EOS
    want = expect()
    assert want[:, 0].tolist() == [sp.EOS, 7, sp.EOS, sp.EOS, sp.EOS, 7, sp.EOS, sp.EOS] and (want[:, 1:] == 7).all()
    assert h.run(slabs, kw)[0] == 0
    assert np.array_equal(h.tokens(), want)
    # the hold-off mask act[b]
    act = np.array([0, 0, 1, 0, 1, 0, 0, 1])
    h.act.copy_(torch.from_numpy(act).int())
    want = expect(act=act)
    assert want[:, 0].tolist() == [sp.EOS, 7, 7, sp.EOS, 7, 7, sp.EOS, 7]
    assert h.run(slabs, kw)[0] == 0
    assert np.array_equal(h.tokens(), want)
    # draw 1: the rows with a new EOS (tok0 == EOS, not in EOS mode) lose it; row 6 is in EOS mode already
    h.act.zero_()
    assert h.run(slabs, kw)[0] == 0
    h.eos_mode[6] = 1
    new = np.array([1, 0, 1, 1, 1, 0, 0, 1])
    assert np.array_equal(h.tokens()[:, 0] == sp.EOS, new | (np.arange(B) == 6))
    want = expect(new_eos=new)
    assert want[:, 0].tolist() == [7, 7, 7, 7, 7, 7, sp.EOS, 7]
    assert h.run(slabs, kw, draw=1)[0] == 0
    assert np.array_equal(h.tokens(draw=1), want)
    # force_full_length
    h.eos_mode.zero_()
    want = expect(force_full_length=True)
    assert (want == 7).all()
    assert h.run(slabs, kw, ffl=1)[0] == 0
    assert np.array_equal(h.tokens(), want)
    # prefill: no bias, EOS open on every codebook
    want = expect(prefill=True)
    assert (want == sp.EOS).all()
    assert h.run(slabs, kw, prefill=1)[0] == 0
    assert np.array_equal(h.tokens(), want)
    # draw 1 without a new EOS in any row, and any call with the done word set, write nothing
    h.tok0.fill_(POISON)
    h.tok1.fill_(POISON)
    assert h.run(slabs, kw, draw=1)[0] == 0
    assert (h.tok0 == POISON).all() and (h.tok1 == POISON).all()
    h.set_scal(offset=4, step=2, done=1)
    h.tok0[0] = sp.EOS                           # (a new EOS, so only the done word stops the resample)
    assert h.run(slabs, kw)[0] == 0 and h.run(slabs, kw, draw=1)[0] == 0
    assert h.tok0[0] == sp.EOS and (h.tok0[1:] == POISON).all() and (h.tok1 == POISON).all()


# ---------------------------------------------------------------------------- the window contract
@pytest.mark.parametrize("window,gen_len", [(0, 513), (513, 513), (600, 1000), (100000, 514)])
def test_logits_entries_refuse_a_window_beyond_512(window, gen_len):
    B, K, V = 2, 2, 1026
    lg = torch.zeros(B, K, V, device=DEV)
    gen = torch.full((B, K, gen_len), 7, dtype=torch.int64, device=DEV)
    rp = torch.full((B,), 2.0, device=DEV)
    out = torch.full((B, K), POISON, dtype=torch.int64, device=DEV)
    par = _params(dict(temperature=0.0, repetition_penalty_window=window))
    stride, _ = zs.torch_noise_policy(B * K * V, DEV)
    for entry, tail in (("zk_sample_logits", (1, 0, 0, 0)), ("zk_sample_logits_torch", (1, 0, stride))):
        rc, msg = _rc(entry, ptr(lg), B, K, V, ptr(gen), gen_len, gen_len, ptr(rp), C.byref(par), *tail, ptr(out),
                      _lib.stream_ptr(lg.device))
        torch.cuda.synchronize()
        assert rc != 0 and entry + ": repetition window" in msg and "512" in msg, (rc, msg)
        assert (out == POISON).all()                     # nothing was launched
    with pytest.raises(_lib.ZonosHipError, match="repetition window"):
        zs.sample_from_logits(lg, temperature=0.0, generated_tokens=gen, repetition_penalty_window=window, seed=1)


@pytest.mark.parametrize("gen_stride,gen_len", [(8, 9), (8, -1), (0, 1)])
def test_logits_entries_refuse_a_history_length_outside_the_buffer(gen_stride, gen_len):
    """0 <= gen_len <= gen_stride (include/zonos_hip.h): anything else is an error return, nothing launched."""
    B, K, V = 2, 2, 1026
    lg = torch.zeros(B, K, V, device=DEV)
    gen = torch.full((B, K, 8), 7, dtype=torch.int64, device=DEV)
    rp = torch.full((B,), 2.0, device=DEV)
    out = torch.full((B, K), POISON, dtype=torch.int64, device=DEV)
    par = _params(dict(temperature=0.0, repetition_penalty_window=2))
    stride, _ = zs.torch_noise_policy(B * K * V, DEV)
    for entry, tail in (("zk_sample_logits", (1, 0, 0, 0)), ("zk_sample_logits_torch", (1, 0, stride))):
        rc, msg = _rc(entry, ptr(lg), B, K, V, ptr(gen), gen_stride, gen_len, ptr(rp), C.byref(par), *tail, ptr(out),
                      _lib.stream_ptr(lg.device))
        torch.cuda.synchronize()
        assert rc != 0 and entry + ": gen_len" in msg, (rc, msg)
        assert (out == POISON).all()


def test_logits_entries_take_the_windows_that_fit(fam):
    """rp_window 0 (the whole history), a window beyond the history, 512 of 700 columns: against the reference,
    on both entries (the torch entry draws nothing at temperature 0)."""
    names = {"W0-len12", "W0-len300", "W600-len20", "W512-len700"}
    cases = [c for c in fam["greedy_rp"] if c.name in names]
    assert len(cases) == len(names)
    for c in cases:
        assert not _flips(c, _sample(c, **c.coords)), c.name
        g = torch.Generator(device=DEV)
        g.manual_seed(1)
        assert not _flips(c, _sample(c, generator=g)), c.name
        assert int(g.get_offset()) == 0


@pytest.mark.parametrize("window", [0, 513, -1])
def test_heads_entry_refuses_the_window(window):
    B, K, V = 2, 2, 1026
    h = Heads(B, K, V, Ld=8)
    h.set_scal(offset=4, step=2)
    slabs = np.zeros((1, 2 * B, K * V), dtype=np.float32)
    for prefill, draw in ((0, 0), (0, 1), (1, 0)):
        rc, msg = h.run(slabs, dict(temperature=0.0, repetition_penalty_window=window), prefill=prefill, draw=draw)
        assert rc != 0 and "zk_sample_heads: repetition window" in msg, (rc, msg)
    assert (h.tok0 == POISON).all() and (h.tok1 == POISON).all()
    assert h.run(slabs, dict(temperature=0.0, repetition_penalty_window=512))[0] == 0


@pytest.mark.parametrize("window", [0, 513])
def test_generate_refuses_the_window(window):
    from zonos_amd.engine import EngineConfig, HipDecoder

    from .golden_util import TINY, load_gen_case
    c = load_gen_case("greedy")
    eng = HipDecoder(EngineConfig(TINY.d_model, TINY.n_layer, TINY.n_heads, TINY.n_kv, TINY.d_ff), c["W"], DEV)
    with pytest.raises(ValueError, match="repetition_penalty_window"):
        eng.generate(c["cond"].to(DEV), c["prefix"].to(DEV), 4, 2.0, c["B"],
                     dict(c["sp"], repetition_penalty_window=window), seed=c["seed"])
