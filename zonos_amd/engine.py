"""The MI355X decode engine: Zonos.generate()'s hot loop on hand-written HIP kernels.

Restates zonos/model.py:224-457 (generate) with the transformer backbone of
zonos/backbone/_torch.py, the heads/CFG of model.py:100-116, the sampler of
zonos/sampling.py and the delay pattern of zonos/codebook_pattern.py.

Design (MI355X-first):
  * All per-step state (offset, position, EOS protocol, repetition penalty, delayed
    codes) lives on the device; one decode step = a fixed launch sequence with no host
    synchronisation, captured once into a hipGraph and replayed in chunks of
    `poll_every` steps. The host polls a `done` word between chunks; steps after
    completion are no-ops (every kernel checks the word).
  * Weights are bf16 in HBM in the engine's layouts: 9 embedding tables stacked
    [9][1026][D], the 9 heads stacked [9*1026][D], fc1 rows interleaved for the fused
    SwiGLU epilogue, GEMM weights fragment-packed (zk_pack_weights). The KV cache stores
    per (row, kv head) 32-key slices in MFMA-fragment order (zonos_amd.kvlayout), in bf16 or,
    opt-in (generate(kv_dtype="fp8") / ZONOS_KV_DTYPE=fp8), as e4m3fn bytes with one power-of-two
    scale per key: half the KV memory and half the bytes the decode attention streams. Likewise opt-in
    (generate(weight_dtype="fp8") / ZONOS_WEIGHT_DTYPE=fp8): the four linear weights of every block as
    e4m3fn bytes with one power-of-two scale per output row (zonos_amd.wlayout), streamed by the B <= 8
    step's GEMVs in place of the bf16 images, which stay for the prefill.
  * torch is plumbing only: it allocates device memory and provides the stream.
"""
from __future__ import annotations

import ctypes as C
import logging
import math
import os
import weakref
from dataclasses import dataclass
from types import SimpleNamespace

import torch

from . import _lib
from . import requests as zrequests
from . import sampling as zsampling
from ._lib import GenState, SamplingParams, call, ptr

EOS, MASK, UNKNOWN = 1024, 1025, -1
KV_DTYPES = ("bf16", "fp8")
WEIGHT_DTYPES = ("bf16", "fp8")
RP_WINDOW_MAX = 512          # sampler.hip MAXW: the repetition-penalty window the sampler holds in LDS


def resolve_kv_dtype(kv_dtype: str | None) -> str:
    """generate()'s ``kv_dtype``: None reads the environment variable ZONOS_KV_DTYPE (default bf16)."""
    if kv_dtype is None:
        kv_dtype = os.environ.get("ZONOS_KV_DTYPE") or "bf16"
    if kv_dtype not in KV_DTYPES:
        raise ValueError(f"kv_dtype must be one of {KV_DTYPES}, not {kv_dtype!r}")
    return kv_dtype


def resolve_weight_dtype(weight_dtype: str | None) -> str:
    """generate()'s ``weight_dtype``: None reads the environment variable ZONOS_WEIGHT_DTYPE (default bf16)."""
    if weight_dtype is None:
        weight_dtype = os.environ.get("ZONOS_WEIGHT_DTYPE") or "bf16"
    if weight_dtype not in WEIGHT_DTYPES:
        raise ValueError(f"weight_dtype must be one of {WEIGHT_DTYPES}, not {weight_dtype!r}")
    return weight_dtype


def check_sampling_params(spd: dict) -> None:
    """generate()'s refusals of sampling parameters the sampler would not treat as the reference does. The
    reference slices generated[..., -window:] (sampling.py:142): a window of 0 is the whole history, which
    outgrows the sampler's window during generation (zk_sample_heads refuses the same values)."""
    rpw = int(spd["repetition_penalty_window"])
    if not 1 <= rpw <= RP_WINDOW_MAX:
        raise ValueError(f"repetition_penalty_window={rpw} must be in [1, {RP_WINDOW_MAX}]: 0 penalises the "
                         f"whole history in the reference (it does not switch the penalty off; "
                         f"repetition_penalty=1.0 does) and the sampler holds {RP_WINDOW_MAX} columns")


N_CB = 9
VOCAB = 1026
ATTN_CHUNK = 256


# ---------------------------------------------------------------------- streaming (DESIGN §6 "Streaming")
def stream_plan(P: int, C: int, H: int, upto_prev: int, upto: int, ended: bool) -> list:
    """The chunks to emit at a poll that found frames < ``upto`` final, the poll before having found ``upto_prev``
    (anything <= P before the first poll): a list of windows (f0, c0, c1, f1) in absolute code frames.

    Chunk j covers [c0, c1) = [P + j C, P + (j + 1) C) and is decoded inside [f0, f1) = [max(P, c0 - H),
    min(c1 + H, upto)): H frames of context on each side (DacSpec.halo_frames), none before P -- the streamed audio
    is the decode of the returned codes, which do not hold the audio prefix -- and none past the final frames. It is
    ready once c1 + H <= upto. ``ended`` (the loop has stopped, ``upto`` is final) flushes every remaining frame,
    a short last chunk included. Pure host arithmetic; every frame of [P, final upto) is covered exactly once."""
    if C < 1 or H < 0 or P < 0:
        raise ValueError(f"stream_plan: C={C} must be >= 1, H={H} and P={P} >= 0")

    def ready(u):                # chunks j with P + (j + 1) C + H <= u
        return max(0, (u - H - P) // C)

    j1 = max(ready(upto_prev), -(-(upto - P) // C)) if ended else ready(upto)
    out = []
    for j in range(ready(upto_prev), j1):
        c0 = P + j * C
        c1 = min(c0 + C, upto)
        out.append((max(P, c0 - H), c0, c1, min(c1 + H, upto)))
    return out


@dataclass
class StreamChunk:
    """One item of HipDecoder.stream(): ``index`` counts chunks from 0; ``frame0`` is the chunk's first code frame
    in the coordinates of the returned codes (the audio prefix not counted); ``wavs[b]`` the fp32 [1, n_b] samples
    of utterance b (n_b = 0 once it has ended); ``done[b]`` says that utterance b has no audio behind this chunk."""
    index: int
    frame0: int
    wavs: list
    done: list


class _Streamer:
    """The device side of stream(): window decodes on a second HIP stream, chunks handed out through one pinned
    buffer. The decode of the windows a poll made ready is enqueued after the next poll's graph launch, behind an
    event recorded after its own poll, so the decode steps never wait for the DAC; the window kernel reads final
    columns only, which later steps do not rewrite."""

    def __init__(self, decoder, B: int, C: int, to_host: bool, device):
        self.dec, self.B, self.C, self.to_host = decoder, B, C, to_host
        self.H = decoder.spec.halo_frames
        self.hop = decoder.spec.hop_length
        self.device = device
        self.main = torch.cuda.current_stream(device)
        self.side = torch.cuda.Stream(device)
        self.copied = torch.cuda.Event()
        self.meta = torch.empty(2, B, dtype=torch.int32, device=device)
        self.pin_meta = torch.empty(2, B, dtype=torch.int32).pin_memory()
        if to_host:
            self.chunk = torch.empty(B * C * self.hop, device=device)
            self.pin = torch.empty(B * C * self.hop).pin_memory()
        self.index = 0
        self.steps = 0               # decode steps run when the chunk last yielded became ready
        self.upto_prev = 0
        self.decode_events = None    # tools/stream_bench.py: a list collects (start, end) events per window

    def mark(self):
        """An event behind what the main stream holds now (the poll just launched)."""
        ev = torch.cuda.Event()
        ev.record(self.main)
        return ev

    def plan(self, P: int, upto: int, ended: bool, steps: int, ev) -> dict:
        wins = stream_plan(P, self.C, self.H, self.upto_prev, upto, ended)
        self.upto_prev = max(self.upto_prev, upto)
        return dict(wins=wins, P=P, upto=upto, ended=ended, steps=steps, ev=ev)

    def emit(self, delayed: torch.Tensor, p: dict):
        """Decode and yield the windows of plan p, one StreamChunk each."""
        B, hop = self.B, self.hop
        for f0, c0, c1, f1 in p["wins"]:
            n = B * (c1 - c0) * hop
            with torch.cuda.stream(self.side):
                if p["ev"] is not None:
                    self.side.wait_event(p["ev"])
                else:
                    self.side.wait_stream(self.main)
                buf = self.chunk if self.to_host else torch.empty(n, device=self.device)
                if self.decode_events is not None:
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record(self.side)
                self.dec.decode_window(delayed, p["P"], f0, c0, c1, f1, p["upto"], chunk=buf, meta=self.meta)
                if self.decode_events is not None:
                    t1.record(self.side)
                    self.decode_events.append((t0, t1))
                if self.to_host:
                    self.pin[:n].copy_(buf[:n], non_blocking=True)
                self.pin_meta.copy_(self.meta, non_blocking=True)
                self.copied.record(self.side)
            self.copied.synchronize()
            nb, end = self.pin_meta[0].tolist(), self.pin_meta[1].tolist()
            src = (self.pin if self.to_host else buf)[:n].view(B, (c1 - c0) * hop)
            wavs = [src[b:b + 1, :nb[b]].clone() if self.to_host else src[b:b + 1, :nb[b]] for b in range(B)]
            last = p["ended"] and c1 >= p["upto"]
            done = [last or 0 <= end[b] <= c1 for b in range(B)]
            self.steps = p["steps"]
            chunk = StreamChunk(self.index, c0 - p["P"], wavs, done)
            self.index += 1
            yield chunk

    def drain(self):
        self.side.synchronize()


class AudioStream:
    """What HipDecoder.stream() returns: an iterator of StreamChunk. ``steps`` is the number of decode steps that had
    run when the chunk last yielded became ready; after exhaustion ``codes`` holds what generate() returns for the
    same arguments. ``close()`` (or dropping the iterator, or leaving a ``with`` block) ends the generation early:
    what is enqueued is drained and the engine is ready for the next call."""

    def __init__(self, engine, run):
        self._engine, self._run = engine, run
        self._it = engine._decode_loop(run)
        self._started = False
        self.codes = None

    @property
    def steps(self) -> int:
        return self._run.streamer.steps

    def __iter__(self):
        return self

    def __next__(self) -> StreamChunk:
        self._started = True
        try:
            return next(self._it)
        except StopIteration:
            self.codes = self._run.result
            raise

    def close(self):
        self._it.close()
        if not self._started:            # never iterated: the prefill is enqueued all the same
            self._started = True
            self._engine._finish(self._run)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class EngineConfig:
    d_model: int
    n_layer: int
    n_heads: int
    n_kv: int
    d_ff: int
    eps: float = 1e-5

    @property
    def head_dim(self):
        return self.d_model // self.n_heads

    @classmethod
    def from_backbone_config(cls, bc) -> "EngineConfig":
        return cls(d_model=bc.d_model, n_layer=bc.n_layer, n_heads=bc.attn_cfg["num_heads"],
                   n_kv=bc.attn_cfg["num_heads_kv"], d_ff=bc.attn_mlp_d_intermediate, eps=bc.norm_epsilon)


def rope_table(seq_len: int, head_dim: int, base: float = 10000.0) -> torch.Tensor:
    """precompute_freqs_cis (_torch.py:9-15), computed on the host CPU exactly as the
    reference does, then uploaded: [seq_len][hd/2][2] fp32 (cos, sin)."""
    inv = 1.0 / (base ** (torch.arange(0, head_dim, 2)[: head_dim // 2].float() / head_dim))
    ang = torch.outer(torch.arange(seq_len, device=inv.device), inv)
    z = torch.polar(torch.ones_like(ang), ang)
    return torch.stack([z.real, z.imag], dim=-1).contiguous()


def pack_weights(w: torch.Tensor, stream) -> torch.Tensor:
    """nn.Linear bf16 [N][K] -> the GEMM's fragment-packed layout (zk_pack_weights)."""
    N, K = w.shape
    out = torch.empty((N + 63) // 64 * 64, K, dtype=w.dtype, device=w.device)
    call("zk_pack_weights", ptr(w), N, K, ptr(out), stream)
    return out


def unpack_weights(wp: torch.Tensor, N: int) -> torch.Tensor:
    """Inverse of pack_weights: the fragment-packed image [ceil64(N)][K] -> nn.Linear order bf16 [N][K]."""
    Np, K = wp.shape
    x = wp.reshape(Np // 16, K // 32, 4, 16, 8)               # tile kc lg ln e  (lane = 16 lg + ln)
    return x.permute(0, 3, 1, 2, 4).reshape(Np, K)[:N].contiguous()


def pack_weights_e4m3(w: torch.Tensor, stream) -> tuple[torch.Tensor, torch.Tensor]:
    """nn.Linear bf16 [N][K] -> (packed e4m3fn image uint8 [ceil64(N) * K], scale bytes uint8 [ceil64(N)]):
    zk_pack_weights_e4m3, bit-identical to wlayout.pack_w8(*wlayout.quantize_w_e4m3(w))."""
    N, K = w.shape
    Np = (N + 63) // 64 * 64
    out = torch.empty(Np * K, dtype=torch.uint8, device=w.device)
    sc = torch.empty(Np, dtype=torch.uint8, device=w.device)
    call("zk_pack_weights_e4m3", ptr(w), N, K, ptr(out), ptr(sc), stream)
    return out, sc


def _split_for(N: int, K: int, M: int, target_blocks: int = 256) -> int:
    """Split-K count for the 128x64-tile GEMM: enough workgroups to cover the CUs.
    Depends on (N, K) only for M <= 128 so the reduction order is batch-invariant."""
    if M > 128:
        return 1
    tiles = (N + 63) // 64
    want = max(1, math.ceil(target_blocks / tiles))
    s = 1
    for cand in range(1, want + 1):
        if K % (cand * 64) == 0:
            s = cand
    return s


def attn_splits_for(R: int, Hkv: int, smax: int, target_blocks: int = 512) -> int:
    """Workgroups per (row, kv head) for flash-decoding. Measured at R=128 (B=64): one
    workgroup per (row, kv head) (512 workgroups, no combine pass) reads 5.4-5.7 TB/s at
    ctx 1.7-3k vs 4.5-4.7 with 2 splits. Small batches split the keys to fill the CUs, but
    each split must cover >= 2048 keys of the cache: the combine launch costs ~6 us, more than
    it saves below that (B=1, 10 s: 1.294 ms per decode step unsplit vs 1.353 with 10 splits;
    such A/Bs run through tools/gpu_ab.sh)."""
    want = -(-target_blocks // (R * Hkv))
    cap = max(1, -(-smax // 2048))
    return max(1, min(want, cap, smax // 128))


def attn_merge_for(R: int, smax: int) -> int:
    """B = 1 (R = 2 rows): key splits of the decode attention whose partials the out_proj GEMV
    merges in its prologue (zk_attn_decode_q_part + zk_gemv_attn_out) -- more CUs stream the
    small KV cache without a combine launch or in-launch tickets. 0 = unsplit attention. The
    splits take 32-key slices in turn (4 waves per split), so any count covers any context."""
    if R > 2:
        return 0
    for v in (16, 8, 4, 2):
        if ATTN_MERGE_DEFAULT >= v and smax >= 128:
            return v
    return 0


# c2 (B=1, Lc=160, 861 tokens) decode step: 1.13 ms unsplit, 1.09 / 1.07 / 1.085 ms with 2 / 4 / 8
# merged splits (profiles/r2_s4_attn_merge_ab.txt)
ATTN_MERGE_DEFAULT = 4


def decode_splits(c, R: int) -> dict:
    """Split-K counts of the decode GEMMs over R rows (prefill runs every GEMM unsplit).
    heads: no split-K (145 workgroups of 64 columns stream 37.8 MB in 15.6 us vs 19.8 us with 2
    splits, tools/microbench.py gemm; the sampler then reads one slab). out_proj: 4-way split-K
    (128 workgroups) is as fast as 8-way (6.6 vs 6.5 us) and halves the fp32 slabs it writes and
    k_resid_ln reads (4.2 vs 8.4 MB; resid_ln 4.3 vs 4.8 us). fc2: of the attention MLP, or of the
    hybrid's Mamba-block MLP (d_mlp) when there is no attention MLP."""
    D, H, hd = c.d_model, c.n_heads, c.head_dim
    return dict(qkv=_split_for((H + 2 * c.n_kv) * hd, D, R), o=_split_for(D, H * hd, R, target_blocks=128),
                fc2=_split_for(D, c.d_ff or getattr(c, "d_mlp", 0) or 64, R), heads=1)


def activation_buffers(c, dev, Mp: int, R: int, smax: int, splits: dict, attn_ways: int) -> dict:
    """The buffers one pass of either backbone works in: a prefill over Mp rows (split-K 1) or a
    decode step over R <= Mp rows under `splits`. part holds the fp32 slabs of whichever GEMM is
    running: Mp rows unsplit or R rows x its split (the heads: R rows only); attn_work the partials
    of attn_ways key splits. A hybrid config adds the fp32 residual (xf), the Mamba y * silu(z) /
    gated-norm rows (yz, ym) and the prefill conv scratch (xc)."""
    D, H, Hk, hd = c.d_model, c.n_heads, c.n_kv, c.head_dim
    di, nin = getattr(c, "d_inner", 0), getattr(c, "d_in_proj", 0)
    f32, bf = torch.float32, torch.bfloat16

    def rows(*names):            # slab rows of the widest of these GEMMs
        return max(Mp, *(splits.get(n, 0) * R for n in names))

    part_n = max((H + 2 * Hk) * hd * rows("qkv"), D * rows("o", "fc2", "out"), nin * rows("inp"),
                 N_CB * VOCAB * splits.get("heads", 0) * R)
    ws = dict(x=torch.empty(Mp, D, dtype=bf, device=dev), xn=torch.empty(Mp, D, dtype=bf, device=dev),
              q=torch.empty(Mp, H * hd, dtype=bf, device=dev), y=torch.empty(Mp, H * hd, dtype=bf, device=dev),
              h=torch.empty(Mp, max(c.d_ff, getattr(c, "d_mlp", 0), 1), dtype=bf, device=dev),
              part=torch.empty(part_n, dtype=f32, device=dev),
              attn_work=torch.empty(max(1, R * Hk * attn_ways * (8 + 4 * hd)), dtype=f32, device=dev),
              scal=torch.zeros(16, dtype=torch.int32, device=dev))
    if di:
        ws.update(xf=torch.empty(Mp, D, dtype=f32, device=dev) if c.residual_in_fp32 else None,
                  yz=torch.empty(Mp, di, dtype=f32, device=dev), ym=torch.empty(Mp, di, dtype=bf, device=dev),
                  xc=torch.empty(Mp, c.conv_dim, dtype=bf, device=dev))
    return ws


def generation_state(dev, B: int, Ld: int) -> dict:
    """The device words of the generate() loop (zk_gen_state) and the sampler's logits copy."""
    f32, i32 = torch.float32, torch.int32
    return dict(eos_mode=torch.zeros(B, dtype=i32, device=dev), steps_after=torch.zeros(B, dtype=i32, device=dev),
                remaining=torch.zeros(B, dtype=i32, device=dev), stopping=torch.zeros(B, dtype=i32, device=dev),
                act=torch.zeros(B, dtype=i32, device=dev), rp=torch.ones(B, dtype=f32, device=dev),
                tok0=torch.zeros(B * N_CB, dtype=i32, device=dev), tok1=torch.zeros(B * N_CB, dtype=i32, device=dev),
                delayed=torch.empty(B, N_CB, Ld, dtype=torch.int64, device=dev),
                dbg=torch.empty(B, N_CB, VOCAB, dtype=f32, device=dev))


class HipBackbone:
    """The 26 transformer blocks + final LayerNorm on the device (zonos/backbone/_torch.py:52-152):
    bf16 weights in the engine's layouts and the layer launch sequence. Shared by the generate()
    engine (HipDecoder) and the backbone plugin (zonos_amd.backbone.HipZonosBackbone)."""

    def __init__(self, cfg: EngineConfig, weights: dict, device="cuda", prefix: str = "backbone."):
        _lib.load()
        self.cfg = cfg
        self.fuse_qkv = True      # in_proj epilogue inside the decode attention launch (False: separate kernel)
        self.rope_neox = 0        # transformer: interleaved RoPE pairs (_torch.py:18-30)
        self.device = torch.device(device)
        c = cfg
        bf = torch.bfloat16
        dev = self.device

        def w(name):
            t = weights[prefix + name]
            return t.to(device=dev, dtype=bf).contiguous()

        stream = _lib.stream_ptr(dev)
        self.layers = []
        for i in range(c.n_layer):
            p = f"layers.{i}."
            fc1 = w(p + "mlp.fc1.weight")
            fc1p = torch.empty_like(fc1)
            call("zk_permute_fc1", ptr(fc1), c.d_ff, c.d_model, ptr(fc1p), stream)
            del fc1
            self.layers.append(dict(
                ln1_w=w(p + "norm.weight"), ln1_b=w(p + "norm.bias"),
                wqkv=pack_weights(w(p + "mixer.in_proj.weight"), stream),
                wo=pack_weights(w(p + "mixer.out_proj.weight"), stream),
                ln2_w=w(p + "norm2.weight"), ln2_b=w(p + "norm2.bias"),
                fc1=pack_weights(fc1p, stream), fc2=pack_weights(w(p + "mlp.fc2.weight"), stream)))
        self.lnf_w = w("norm_f.weight")
        self.lnf_b = w("norm_f.bias")
        self.freqs = rope_table(16384, c.head_dim).to(dev)

    def splits(self, R: int) -> dict:
        return decode_splits(self.cfg, R)

    W8_NAMES = ("wqkv", "wo", "fc1", "fc2")

    def quantize_weights_fp8(self):
        """The FP8 images of the four linear weights of every layer (L[name + "8"], L[name + "_scale"]), made
        once from the bf16 images and kept beside them (+ 50 % of the layer weight memory): fc1 in its
        zk_permute_fc1 order, as the bf16 image holds it."""
        if self.layers and "wqkv8" in self.layers[0]:
            return
        c = self.cfg
        rows = dict(wqkv=(c.n_heads + 2 * c.n_kv) * c.head_dim, wo=c.d_model, fc1=2 * c.d_ff, fc2=c.d_model)
        stream = _lib.stream_ptr(self.device)
        for L in self.layers:
            for name in self.W8_NAMES:
                L[name + "8"], L[name + "_scale"] = pack_weights_e4m3(unpack_weights(L[name], rows[name]), stream)
        torch.cuda.synchronize(self.device)

    def _layers_small(self, ws, R: int, stream, skip):
        """Decode step of the 26 blocks for R <= 16 rows (B <= 8), five launches per block:
        [norm -> in_proj] -> attention (RoPE, KV write) -> [out_proj -> x += .] ->
        [norm2 -> fc1 -> SwiGLU] -> [fc2 -> x += .] (_torch.py:99-102, 117-152). Leaves the
        residual stream in ws['x'] (norm_f runs in the heads GEMV's prologue)."""
        c = self.cfg
        D, H, Hk, hd, Fd = c.d_model, c.n_heads, c.n_kv, c.head_dim, c.d_ff
        Nqkv = (H + 2 * Hk) * hd
        x, y, h, part, scal = ws["x"], ws["y"], ws["h"], ws["part"], ws["scal"]
        merge = ws.get("attn_merge", 0)
        w8 = bool(ws.get("w_fp8"))           # the _w8 entries on the byte images (same sequence, same arithmetic)

        def W(L, name):                      # the weight argument(s) of a GEMV entry
            return (ptr(L[name + "8"]), ptr(L[name + "_scale"])) if w8 else (ptr(L[name]),)

        fused, qkv_rope, attn_out = (n + "_w8" if w8 else n for n in ("zk_gemv_fused", "zk_gemv_qkv_rope",
                                                                       "zk_gemv_attn_out"))
        for i, L in enumerate(self.layers):
            kc, vt = self._kv(ws, i)
            if merge and not self.rope_neox:
                # B = 1: RoPE + KV write in the in_proj epilogue (q -> y), prologue-free attention over
                # 32-key slices, partials merged by the out_proj GEMV
                call(qkv_rope, ptr(x), *W(L, "wqkv"), R, H, Hk, hd, ptr(L["ln1_w"]), ptr(L["ln1_b"]),
                     c.eps, ptr(y), ptr(kc), ptr(vt), ws["smax"], ptr(scal[1:2]), ptr(self.freqs), skip, stream)
                call("zk_attn_decode_q_part", ptr(y), ptr(kc), ptr(vt), R, H, Hk, hd, ws["smax"], 1, ptr(scal[1:2]),
                     ptr(ws["attn_work"]), merge, skip, stream)
                call(attn_out, ptr(ws["attn_work"]), merge, Hk, *W(L, "wo"), R, D, H * hd, ptr(x), skip, stream)
            else:
                call(fused, ptr(x), D, *W(L, "wqkv"), R, Nqkv, D, 0, ptr(L["ln1_w"]), ptr(L["ln1_b"]),
                     c.eps, ptr(part), None, skip, stream)
                if merge:
                    call("zk_attn_decode_qkv_part", ptr(part), 1, ptr(self.freqs), ptr(kc), ptr(vt), R, H, Hk, hd,
                         ws["smax"], 1, ptr(scal[1:2]), ptr(ws["attn_work"]), merge, self.rope_neox, skip, stream)
                    call(attn_out, ptr(ws["attn_work"]), merge, Hk, *W(L, "wo"), R, D, H * hd, ptr(x), skip, stream)
                else:
                    if ws.get("row_off") is not None:    # a ragged request batch: a context per row
                        call("zk_attn_decode_qkv_sc_rows", ptr(part), 1, ptr(self.freqs), ptr(kc), ptr(vt), R, H, Hk,
                             hd, ws["smax"], 1, ptr(scal[1:2]), ptr(ws["row_off"]), ptr(ws["attn_work"]),
                             ws["attn_splits"], ptr(ws["attn_cnt"]), ptr(y), skip, stream)
                    else:
                        call("zk_attn_decode_qkv_sc", ptr(part), 1, ptr(self.freqs), ptr(kc), ptr(vt), R, H, Hk, hd,
                             ws["smax"], 1, ptr(scal[1:2]), ptr(ws["attn_work"]), ws["attn_splits"],
                             ptr(ws["attn_cnt"]), ptr(y), self.rope_neox, skip, stream)
                    call(fused, ptr(y), H * hd, *W(L, "wo"), R, D, H * hd, 2, None, None, c.eps, None,
                         ptr(x), skip, stream)
            call(fused, ptr(x), D, *W(L, "fc1"), R, 2 * Fd, D, 1, ptr(L["ln2_w"]), ptr(L["ln2_b"]),
                 c.eps, None, ptr(h), skip, stream)
            call(fused, ptr(h), Fd, *W(L, "fc2"), R, D, Fd, 2, None, None, c.eps, None, ptr(x), skip,
                 stream)

    def _kv(self, ws, layer):
        if ws.get("kv_fp8"):             # a bf16 kernel must never be pointed at the (half as large) byte caches
            raise ValueError("this workspace holds the FP8 KV cache (bytes + scales, _kv8): "
                             "the bf16 attention entries cannot read it")
        if "kv_layers" in ws:            # caches handed out per layer (backbone plugin)
            kv = ws["kv_layers"][layer]
            return kv[0], kv[1]
        return ws["kv"][layer, 0], ws["kv"][layer, 1]

    def _kv8(self, ws, layer):
        """FP8 cache of a layer: K8 and V8 bytes, K and V scale bytes (zonos_amd.kvlayout)."""
        return ws["kv"][layer, 0], ws["kv"][layer, 1], ws["kv_scale"][layer, 0], ws["kv_scale"][layer, 1]

    # ------------------------------------------------------------------ transformer passes
    def _layers(self, ws, M: int, R: int, S: int, prefill: bool, stream, skip):
        """Run the 26 blocks on xn/x (rows = R*S). Leaves norm_f(x) in ws['xn']."""
        c = self.cfg
        D, H, Hk, hd, Fd = c.d_model, c.n_heads, c.n_kv, c.head_dim, c.d_ff
        Nqkv = (H + 2 * Hk) * hd
        sp = ws["splits"] if not prefill else dict(qkv=1, o=1, fc2=1)
        x, xn, q, y, h, part = ws["x"], ws["xn"], ws["q"], ws["y"], ws["h"], ws["part"]
        scal = ws["scal"]
        pos_dev = None if prefill else ptr(scal[1:2])
        row_off = ws.get("row_off")          # a ragged request batch: the decode attention with a context per row
        if row_off is not None and not prefill and (self.rope_neox or not self.fuse_qkv):
            raise ValueError("a context per row runs the fused decode attention with interleaved RoPE only")
        for i, L in enumerate(self.layers):
            fp8 = bool(ws.get("kv_fp8"))
            kc, vt, ksc, vsc = self._kv8(ws, i) if fp8 else (*self._kv(ws, i), None, None)
            call("zk_gemm_bf16", ptr(xn), D, ptr(L["wqkv"]), M, Nqkv, D, sp["qkv"], 0, ptr(part), None, skip, stream)
            if prefill and fp8:
                # exact prefill on the reusable bf16 scratch pair, then this layer's FP8 cache
                pk, pv = ws["pre_kv"][0], ws["pre_kv"][1]
                call("zk_qkv_rope", ptr(part), sp["qkv"], R, S, H, Hk, hd, ptr(self.freqs), 0, pos_dev, ptr(q),
                     ptr(pk), ptr(pv), ws["pre_smax"], None, 0, skip, stream)
                call("zk_attn_prefill", ptr(q), ptr(pk), ptr(pv), R, S, H, Hk, hd, ws["pre_smax"], ptr(y), stream)
                call("zk_kv_quantize_e4m3", ptr(pk), ptr(pv), R, Hk, hd, S, ws["pre_smax"], ptr(kc), ptr(vt), ptr(ksc),
                     ptr(vsc), ws["smax"], stream)
            elif fp8 and row_off is not None:
                call("zk_attn_decode_qkv_f8_rows", ptr(part), sp["qkv"], ptr(self.freqs), ptr(kc), ptr(vt), ptr(ksc),
                     ptr(vsc), R, H, Hk, hd, ws["smax"], 1, ptr(scal[1:2]), ptr(row_off), ptr(ws["attn_work"]),
                     ws["attn_splits"], ptr(ws["attn_cnt"]), ptr(y), skip, stream)
            elif fp8:
                call("zk_attn_decode_qkv_f8", ptr(part), sp["qkv"], ptr(self.freqs), ptr(kc), ptr(vt), ptr(ksc),
                     ptr(vsc), R, H, Hk, hd, ws["smax"], 1, ptr(scal[1:2]), ptr(ws["attn_work"]), ws["attn_splits"],
                     ptr(ws["attn_cnt"]), ptr(y), skip, stream)
            elif prefill:
                call("zk_qkv_rope", ptr(part), sp["qkv"], R, S, H, Hk, hd, ptr(self.freqs), 0, pos_dev, ptr(q),
                     ptr(kc), ptr(vt), ws["smax"], None, self.rope_neox, skip, stream)
                call("zk_attn_prefill", ptr(q), ptr(kc), ptr(vt), R, S, H, Hk, hd, ws["smax"], ptr(y), stream)
            elif row_off is not None:
                call("zk_attn_decode_qkv_sc_rows", ptr(part), sp["qkv"], ptr(self.freqs), ptr(kc), ptr(vt), R, H, Hk,
                     hd, ws["smax"], 1, ptr(scal[1:2]), ptr(row_off), ptr(ws["attn_work"]), ws["attn_splits"],
                     ptr(ws["attn_cnt"]), ptr(y), skip, stream)
            elif self.fuse_qkv:
                # in_proj epilogue fused into the attention launch (position = ctx - 1 = scal[1])
                # split partials (long contexts at small batch) merged inside the launch
                call("zk_attn_decode_qkv_sc", ptr(part), sp["qkv"], ptr(self.freqs), ptr(kc), ptr(vt), R, H, Hk, hd,
                     ws["smax"], 1, ptr(scal[1:2]), ptr(ws["attn_work"]), ws["attn_splits"],
                     ptr(ws["attn_cnt"]) if "attn_cnt" in ws else None, ptr(y), self.rope_neox, skip, stream)
            else:
                call("zk_qkv_rope", ptr(part), sp["qkv"], R, S, H, Hk, hd, ptr(self.freqs), 0, pos_dev, ptr(q),
                     ptr(kc), ptr(vt), ws["smax"], None, self.rope_neox, skip, stream)
                call("zk_attn_decode", ptr(q), ptr(kc), ptr(vt), R, H, Hk, hd, ws["smax"], 1, ptr(scal[1:2]),
                     ptr(ws["attn_work"]), ws["attn_splits"], ptr(y), skip, stream)
            call("zk_gemm_bf16", ptr(y), H * hd, ptr(L["wo"]), M, D, H * hd, sp["o"], 0, ptr(part), None, skip, stream)
            call("zk_resid_ln", ptr(part), sp["o"], ptr(x), ptr(L["ln2_w"]), ptr(L["ln2_b"]), c.eps, M, D, ptr(x),
                 ptr(xn), 0, skip, stream)
            call("zk_gemm_bf16", ptr(xn), D, ptr(L["fc1"]), M, 2 * Fd, D, 1, 1, None, ptr(h), skip, stream)
            call("zk_gemm_bf16", ptr(h), Fd, ptr(L["fc2"]), M, D, Fd, sp["fc2"], 0, ptr(part), None, skip, stream)
            if i + 1 < len(self.layers):
                nw, nb = self.layers[i + 1]["ln1_w"], self.layers[i + 1]["ln1_b"]
            else:
                nw, nb = self.lnf_w, self.lnf_b
            call("zk_resid_ln", ptr(part), sp["fc2"], ptr(x), ptr(nw), ptr(nb), c.eps, M, D, ptr(x), ptr(xn), 0, skip,
                 stream)


class HipDecoder(HipBackbone):
    """Owns device weights in engine layout and runs generate() on the GPU."""

    # B <= 8 decode (R <= 16 rows) runs each block as five launches (zk_gemv_fused: LayerNorm
    # prologues, residual epilogues, no split-K slabs) instead of seven
    small_batch_path = True
    graph_steps = 1                 # decode steps captured per hipGraph replay (generate's G; 8 measured no faster)
    # layer 0's norm is fused into the embedding kernel (decode) / a zk_layernorm (prefill); False:
    # the subclass runs it as _prenorm (the hybrid backbone's RMS-norm / fp32-residual variants)
    embed_norm = True
    kv_fp8_supported = True         # generate(kv_dtype="fp8"): the transformer backbone only
    _fp8 = False                    # the running generate() uses the FP8 KV cache
    w_fp8_supported = True          # generate(weight_dtype="fp8"): the transformer backbone's small-batch path only
    _w8 = False                     # the running generate() uses the FP8 layer weights
    ragged_supported = True         # generate_requests(ragged=True) with differing lengths: the transformer backbone only

    def __init__(self, cfg: EngineConfig, weights: dict, device="cuda"):
        super().__init__(cfg, weights, device)
        self._load_io(weights)

    def _load_io(self, weights: dict):
        """The 9 embedding tables stacked and the 9 heads stacked + packed (model.py:97-111)."""
        dev = self.device

        def w(name):
            return weights[name].to(device=dev, dtype=torch.bfloat16).contiguous()

        self.emb = torch.stack([w(f"embeddings.{k}.weight") for k in range(N_CB)]).contiguous()
        assert self.emb.shape == (N_CB, VOCAB, self.cfg.d_model), self.emb.shape
        heads = []
        for k in range(N_CB):
            h = w(f"heads.{k}.weight")
            if h.shape[0] < VOCAB:      # pad_weight_ (utils.py:22-37): 1025 -> 1026 rows
                h = torch.cat([h, h.new_zeros(VOCAB - h.shape[0], h.shape[1])])
            heads.append(h)
        self.heads = pack_weights(torch.cat(heads).contiguous(), _lib.stream_ptr(dev))  # [9*1026 -> 9280][D] packed
        self._ws = None
        torch.cuda.synchronize(dev)

    # ------------------------------------------------------------------ workspace
    def _new_state(self, R: int, smax: int) -> dict:
        """What a generate() call starts from zeroed: the KV caches and the in-launch split-combine tickets."""
        c, dev = self.cfg, self.device
        cnt = torch.zeros(R * c.n_kv, dtype=torch.int32, device=dev)
        if self._fp8:      # e4m3fn bytes + one scale byte per (row, kv head, key) for K and for V (kvlayout)
            return dict(kv=torch.zeros(c.n_layer, 2, R * c.n_kv * smax * c.head_dim, dtype=torch.uint8, device=dev),
                        kv_scale=torch.zeros(c.n_layer, 2, R * c.n_kv * smax, dtype=torch.uint8, device=dev),
                        attn_cnt=cnt)
        return dict(kv=torch.zeros(c.n_layer, 2, R * c.n_kv * smax * c.head_dim, dtype=torch.bfloat16, device=dev),
                    attn_cnt=cnt)

    def _alloc(self, B: int, Lc: int, P: int, max_new: int, ragged: bool = False):
        R = 2 * B
        T = P + max_new
        Ld = T + N_CB
        seq_len = Lc + T + N_CB
        smax = -(-seq_len // ATTN_CHUNK) * ATTN_CHUNK
        S_pre = Lc + P + 1
        key = (B, Lc, P, max_new, "ragged" if ragged else "uniform", "fp8" if self._fp8 else "bf16",
               "w8" if self._w8 else "w16")
        if self._ws is not None and self._ws["key"] == key:
            ws = self._ws
            for k in ws["state_keys"]:
                ws[k].zero_()
            return ws
        self.release()
        splits = self.splits(R)
        attn_splits = attn_splits_for(R, self.cfg.n_kv, smax)
        attn_merge = attn_merge_for(R, smax)       # read by the small-batch path only
        state = self._new_state(R, smax)
        ws = dict(key=key, R=R, T=T, Ld=Ld, smax=smax, S_pre=S_pre, splits=splits, attn_splits=attn_splits,
                  attn_merge=attn_merge, state_keys=tuple(state), graph=None, **state,
                  **activation_buffers(self.cfg, self.device, R * S_pre, R, smax, splits, max(attn_splits, attn_merge)),
                  **generation_state(self.device, B, Ld))
        if self._w8:
            ws["w_fp8"] = True
        if self._fp8:
            # the bf16 K / V^T pair the exact prefill of one layer runs on (zeroed once: the prefill attention
            # multiplies the masked tail of its last 32-key slice by p = 0)
            c = self.cfg
            ws["kv_fp8"] = True
            ws["pre_smax"] = -(-S_pre // 128) * 128
            ws["pre_kv"] = torch.zeros(2, R * c.n_kv * ws["pre_smax"] * c.head_dim, dtype=torch.bfloat16,
                                       device=self.device)
        self._ws = ws
        return ws

    def release(self):
        if self._ws is not None and self._ws.get("graph"):
            call("zk_graph_destroy", self._ws["graph"])
        self._ws = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    def _heads(self, ws, R: int, S: int, stream, skip):
        """Heads GEMM on the last position of every row -> split-K slabs in ws['part']. The prefill of a ragged
        request batch (S > 1, ws["row_off"]): on each row's last VALID position, gathered into ws["y"]."""
        D = self.cfg.d_model
        last = ws["xn"][S - 1:]           # rows r*S + S-1 via lda = S*D
        if S > 1 and ws.get("row_off") is not None:
            call("zk_gather_last_rows", ptr(ws["xn"]), R, S, D, ptr(ws["row_off"]), ptr(ws["y"]), stream)
            last, S = ws["y"], 1
        call("zk_gemm_bf16", ptr(last), S * D, ptr(self.heads), R, N_CB * VOCAB, D, ws["splits"]["heads"], 0,
             ptr(ws["part"]), None, skip, stream)

    def _gen_state(self, ws, B, seed, row_base, noise=(0, 0, 0, 0)) -> GenState:
        """noise = (mode, Philox offset, grid-stride, offset per call): zk_gen_state's noise words."""
        return GenState(ptr(ws["scal"]), ptr(ws["eos_mode"]), ptr(ws["steps_after"]), ptr(ws["remaining"]),
                        ptr(ws["stopping"]), ptr(ws["act"]), ptr(ws["rp"]), ptr(ws["tok0"]), ptr(ws["tok1"]),
                        ptr(ws["delayed"]), B, N_CB, ws["Ld"], VOCAB, seed & 0xFFFFFFFFFFFFFFFF, row_base, *noise)

    # the step's launch sequence is enqueued by the C ABI (zk_decode_step); False runs the same
    # sequence from Python (bit-identical; kept as the reference for the test)
    c_step = True

    def _step_desc(self, ws, B, st, sp):
        """zk_step_desc of this workspace: per-layer weights + KV caches, buffers, state, params."""
        c = self.cfg
        if "step_layers" not in ws:
            arr = (_lib.StepLayer * c.n_layer)()
            for i, L in enumerate(self.layers):
                kc, vt, ksc, vsc = self._kv8(ws, i) if ws.get("kv_fp8") else (*self._kv(ws, i), None, None)
                # the FP8 images and scales: NULL before the first FP8 generate() has made them
                w8 = [ptr(L.get(n + sfx)) for sfx in ("8", "_scale") for n in self.W8_NAMES]
                arr[i] = _lib.StepLayer(ptr(L["ln1_w"]), ptr(L["ln1_b"]), ptr(L["wqkv"]), ptr(L["wo"]),
                                        ptr(L["ln2_w"]), ptr(L["ln2_b"]), ptr(L["fc1"]), ptr(L["fc2"]), ptr(kc), ptr(vt),
                                        ptr(ksc), ptr(vsc), *w8)
            ws["step_layers"] = arr
        sps = ws["splits"]
        return _lib.StepDesc(B, c.n_layer, c.d_model, c.n_heads, c.n_kv, c.head_dim, c.d_ff, ws["smax"],
                             sps["qkv"], sps["o"], sps["fc2"], sps["heads"], ws["attn_splits"],
                             ws.get("attn_merge", 0), self.rope_neox, int(self._small(2 * B)), c.eps,
                             int(bool(ws.get("kv_fp8"))), C.cast(ws["step_layers"], C.c_void_p), ptr(self.emb), ptr(self.heads), ptr(self.lnf_w),
                             ptr(self.lnf_b), ptr(self.freqs), ptr(ws["x"]), ptr(ws["xn"]), ptr(ws["y"]), ptr(ws["h"]),
                             ptr(ws["part"]), ptr(ws["attn_work"]), ptr(ws["attn_cnt"]), ptr(ws["dbg"]), st, sp,
                             ptr(ws["pre_kv"][0]) if "pre_kv" in ws else None,
                             ptr(ws["pre_kv"][1]) if "pre_kv" in ws else None, ws.get("pre_smax", 0),
                             int(bool(ws.get("w_fp8"))), ptr(ws.get("rows")))

    def _c_decode(self, ws, B, st, sp, stream):
        if ws.get("row_off") is not None:   # a ragged request batch: the same sequence with a context per row
            call("zk_decode_step_rows", C.byref(self._step_desc(ws, B, st, sp)), ptr(ws["row_off"]), stream)
            return
        call("zk_decode_step", C.byref(self._step_desc(ws, B, st, sp)), stream)

    def _c_prefill(self, ws, B, st, sp, cond, Lc, P, stream):
        if ws.get("row_off") is not None:
            call("zk_prefill_rows", C.byref(self._step_desc(ws, B, st, sp)), ptr(cond), Lc, P, ptr(ws["q"]),
                 ptr(ws["row_off"]), stream)
            return
        call("zk_prefill", C.byref(self._step_desc(ws, B, st, sp)), ptr(cond), Lc, P, ptr(ws["q"]), stream)

    def _decode_step(self, ws, B, st, sp, stream):
        c = self.cfg
        R = 2 * B
        if self.c_step:
            self._c_decode(ws, B, st, sp, stream)
            return
        scal = ws["scal"]
        skip = ptr(scal[3:4])
        L0 = self.layers[0]
        small = self._small(R)                       # layer 0's LayerNorm runs in the in_proj prologue
        own = small or not self.embed_norm           # ... or its own launch (hybrid config variants)
        call("zk_embed_codes", ptr(ws["delayed"]), B, 1, N_CB, ws["Ld"] * N_CB, ws["Ld"], ptr(scal[0:1]), -1,
             ptr(self.emb), VOCAB, c.d_model, 2, ptr(ws["x"]), 1, 0, None if own else ptr(L0["ln1_w"]),
             None if own else ptr(L0["ln1_b"]), c.eps, None if own else ptr(ws["xn"]), skip, stream)
        if not self.embed_norm:
            self._prenorm(ws, R, stream, skip)
        logits, nsp = ws["part"], ws["splits"]["heads"]
        if small:
            self._layers_small(ws, R, stream, skip)
            # heads with the final LayerNorm (norm_f) as the GEMV prologue: one fp32 slab
            call("zk_gemv_fused", ptr(ws["x"]), c.d_model, ptr(self.heads), R, N_CB * VOCAB, c.d_model, 0,
                 ptr(self.lnf_w), ptr(self.lnf_b), c.eps, ptr(ws["part"]), None, skip, stream)
        else:
            self._layers(ws, R, R, 1, False, stream, skip)
            self._heads(ws, R, 1, stream, skip)
        self._sample(ws, logits, nsp, st, sp, 0, 0, stream)

    def _sample(self, ws, logits, nsp, st, sp, prefill: int, prefix_len: int, stream):
        """The step's tail: the sampler draw(s) and the EOS protocol -- batch-wide, or with a request batch
        (ws["rows"]) the rows-mode entries on its per-utterance parameters."""
        rows = ws.get("rows")
        if rows is not None:
            call("zk_sample_heads_rows", ptr(logits), nsp, C.byref(st), ptr(rows), prefill, 0, ptr(ws["dbg"]), stream)
            if not prefill:
                call("zk_sample_heads_rows", ptr(logits), nsp, C.byref(st), ptr(rows), 0, 1, None, stream)
            call("zk_eos_step_rows", C.byref(st), prefill, prefix_len, stream)
            return
        call("zk_sample_heads", ptr(logits), nsp, C.byref(st), C.byref(sp), prefill, 0, ptr(ws["dbg"]), stream)
        if not prefill:
            call("zk_sample_heads", ptr(logits), nsp, C.byref(st), C.byref(sp), 0, 1, None, stream)
        call("zk_eos_step", C.byref(st), prefill, prefix_len, stream)

    def _small(self, R: int) -> bool:
        # (the FP8 KV cache runs the seven-launch sequence at any batch size)
        return self.small_batch_path and R <= 16 and self.cfg.d_model == 2048 and not self._fp8

    # ------------------------------------------------------------------ generate
    @torch.inference_mode()
    def generate(self, prefix_conditioning: torch.Tensor, audio_prefix_codes=None, max_new_tokens: int = 86 * 30,
                 cfg_scale: float = 2.0, batch_size: int = 1, sampling_params: dict | None = None,
                 seed: int = 0, row_base: int = 0, force_full_length: bool = False, callback=None,
                 progress=None, poll_every: int = 16, trace: dict | None = None, use_graph: bool = True,
                 _after_prefill=None, noise: str = "keyed", generator: torch.Generator | None = None,
                 pad_rows: int = 0, kv_dtype: str | None = None, *, weight_dtype: str | None = None):
        """Zonos.generate (model.py:224-457). Returns the list of int64 [9, T_i] code tensors.

        ``weight_dtype``: "bf16" (default) or "fp8" -- the four linear weights of every block as e4m3fn bytes
        with one power-of-two scale per output row (zonos_amd.wlayout), streamed by the GEMVs of the B <= 8
        decode step: half the weight bytes per step. The first such call quantises the weights once and keeps
        the images beside the bf16 ones (the prefill, the heads and the embeddings stay bf16). None reads the
        environment variable ZONOS_WEIGHT_DTYPE. ValueError where the small-batch path does not run: B > 8,
        d_model != 2048, together with kv_dtype="fp8", the hybrid engine.

        ``kv_dtype``: "bf16" (default) or "fp8" -- the KV cache as e4m3fn bytes with one power-of-two scale
        per (row, kv head, key) (zonos_amd.kvlayout): half the KV memory and half the bytes the decode
        attention streams; the prefill stays exact and only the cached keys / values are quantised. None
        reads the environment variable ZONOS_KV_DTYPE. Transformer backbone with head_dim 128 only.

        ``noise`` picks the race noise of the sampler: "keyed" = the engine's stream keyed by
        (seed, step, draw, row_base + b, codebook, token), independent of batch sharding; "torch" =
        torch's own GPU stream, the values the reference's `exponential_` draws from ``generator``
        (default: torch's CUDA generator of the device) -- the generator is read at the start and
        advanced by the Philox offset the reference's sampler calls would have consumed, so
        ``torch.manual_seed(s)`` followed by this call leaves torch's RNG where the reference leaves it.

        ``trace`` (optional dict) receives per-step fp32 CFG logits (before bias) and the
        sampled frames -- test instrumentation, forces one step per poll and no graph.

        ``pad_rows``: the last ``pad_rows`` utterances are padding (generate_sharded's uniform shards)
        whose codes the caller drops. They run through the GEMMs like any row but stay out of the
        batch-wide EOS protocol (model.py:376-393): they start in EOS mode with no hold-off and no
        remaining steps, so an EOS they sample never triggers the resample draw of the real rows and
        never keeps the loop running after the real rows have stopped."""
        run = self._begin(prefix_conditioning, audio_prefix_codes, max_new_tokens, cfg_scale, batch_size,
                          sampling_params, seed, row_base, force_full_length, callback, progress, poll_every, trace,
                          use_graph, _after_prefill, noise, generator, pad_rows, kv_dtype, weight_dtype)
        for _ in self._decode_loop(run):
            pass
        return run.result

    @torch.inference_mode()
    def generate_requests(self, requests, *, callback=None, progress=None, poll_every: int = 16,
                          use_graph: bool = True, trace: dict | None = None, kv_dtype: str | None = None,
                          weight_dtype: str | None = None, ragged: bool = False, _pad: int = 0,
                          _pad_fill: float = 0.0) -> list:
        """A batch of independent requests (zonos_amd.requests.Request): each with its own sampling parameters,
        cfg_scale, seed, noise key, length budget and force_full_length. Returns one int64 [9, T_b] code tensor per
        request: exactly what ``generate(cond_b, prefix_b, n_b, cfg_b, 1, params_b, seed=seed_b, row_base=key_b,
        force_full_length=ffl_b)`` returns, whatever else shares the batch and whichever slot the request takes
        (within one kernel regime: `gemm_regime`, `attn_splits_for`, the dtype options). generate()'s step on the
        rows-mode sampler and EOS kernels (DESIGN §6 "Request batches"); keyed noise only.

        Every request needs the same audio-prefix length and, unless ``ragged=True``, the same conditioning length.
        ``ragged=True``: conditionings of different lengths, each row left-aligned with its own KV position and
        context (DESIGN §6 "Ragged request batches") -- no pad token is attended to, and the statement above holds
        for the request with ITS conditioning. Transformer backbone with interleaved RoPE only; with equal lengths
        it is the default path. The loop runs until the last
        request has ended: a request that ended earlier keeps its row in the launches. ValueError, before anything
        is allocated, for an empty list, ragged prompts, cfg_scale == 1 or a repetition window outside [1, 512].
        ``callback`` / ``progress`` / ``poll_every`` / ``use_graph`` / ``trace`` / ``kv_dtype`` / ``weight_dtype``
        as in generate(). ``_pad``: the last ``_pad`` requests are padding (generate_sharded_requests).
        ``_pad_fill`` (test hook): the value written in place of zero into the padding of a ragged batch -- the
        padded conditioning and, where this class issues the prefill itself (c_step False), the positions of x
        behind it; zk_prefill_rows zeroes those itself."""
        plan = zrequests.plan_requests(requests, self.cfg.d_model, pad=_pad, ragged=ragged)
        if plan.row_off is not None and not (self.ragged_supported and not self.rope_neox):
            raise ValueError(f"ragged=True with conditionings of different lengths needs the transformer backbone "
                             f"with interleaved RoPE ({type(self).__name__}); equal lengths run everywhere")
        cond = zrequests.stack_conditioning(plan, _pad_fill).to(self.device)
        prefix = zrequests.stack_prefixes(plan)
        r0 = plan.requests[0]
        run = self._begin(cond, prefix, plan.max_new, r0.cfg_scale, len(plan.requests), plan.params[0], 0, 0,
                          bool(r0.force_full_length), callback, progress, poll_every, trace, use_graph, None, "keyed",
                          None, 0, kv_dtype, weight_dtype, rows=plan, pad_fill=_pad_fill)
        for _ in self._decode_loop(run):
            pass
        return run.result

    def stream(self, prefix_conditioning: torch.Tensor, audio_prefix_codes=None, max_new_tokens: int = 86 * 30,
               cfg_scale: float = 2.0, batch_size: int = 1, sampling_params: dict | None = None, seed: int = 0,
               row_base: int = 0, force_full_length: bool = False, progress=None, use_graph: bool = True,
               noise: str = "keyed", generator: torch.Generator | None = None, pad_rows: int = 0,
               kv_dtype: str | None = None, *, weight_dtype: str | None = None, autoencoder=None,
               chunk_frames: int = 16, to_host: bool = True) -> AudioStream:
        """generate() that hands out audio while it runs: an iterator of StreamChunk (``chunk_frames`` code frames
        of every utterance each, the last one shorter), decoded by ``autoencoder`` (a DACAutoencoder or a
        HipDacDecoder) from the frames that are final at each poll. generate()'s arguments without ``callback`` /
        ``trace``; the loop is generate()'s with ``poll_every = chunk_frames``, so the codes -- ``.codes`` of the
        returned AudioStream after exhaustion -- and the state torch's generator is left in are generate()'s.

        The chunks of a row, concatenated, are bit for bit ``autoencoder.decode(codes_row[None])[0]``: each chunk
        is decoded inside a window with ``DacSpec.halo_frames`` frames of context on each side. That is the raw
        decoder output: the loudness normalisation, silence trim and fades of ``codes_to_wavs`` need the whole
        utterance and are not applied. ``to_host``: CPU tensors, copied through one pinned buffer (default), or
        device tensors. The prefill is enqueued by this call; the first chunk is ready at the first poll with
        chunk_frames + halo_frames final frames. Ending the iteration early is safe (AudioStream.close)."""
        if int(chunk_frames) < 1:
            raise ValueError(f"chunk_frames={chunk_frames} must be >= 1")
        if autoencoder is None:
            raise ValueError("stream() needs the autoencoder that decodes the chunks")
        decoder = getattr(autoencoder, "decoder", autoencoder)
        with torch.inference_mode():
            run = self._begin(prefix_conditioning, audio_prefix_codes, max_new_tokens, cfg_scale, batch_size,
                              sampling_params, seed, row_base, force_full_length, None, progress, int(chunk_frames),
                              None, use_graph, None, noise, generator, pad_rows, kv_dtype, weight_dtype)
            run.streamer = _Streamer(decoder, batch_size, int(chunk_frames), to_host, self.device)
        out = AudioStream(self, run)
        self._streaming = weakref.ref(out)
        return out

    def _begin(self, prefix_conditioning, audio_prefix_codes, max_new_tokens, cfg_scale, batch_size, sampling_params,
               seed, row_base, force_full_length, callback, progress, poll_every, trace, use_graph, _after_prefill,
               noise, generator, pad_rows, kv_dtype, weight_dtype, rows=None, pad_fill=0.0) -> SimpleNamespace:
        """generate() up to its decode loop: the refusals, the workspace, the prefill and the captured step.
        ``rows`` (generate_requests): the plan of a request batch (zonos_amd.requests.plan_requests) -- the
        batch-wide sampling arguments are then those of request 0 and only feed the debug loggers."""
        assert cfg_scale != 1, "TODO: add support for cfg_scale=1"                     # model.py:247
        if batch_size * 2 != prefix_conditioning.shape[0]:                            # model.py:249-250
            raise ValueError(f"Batch size mismatch: {batch_size} * 2 != {prefix_conditioning.shape[0]}")
        if not 0 <= pad_rows < batch_size:
            raise ValueError(f"pad_rows={pad_rows} must leave at least one real utterance of {batch_size}")
        kv_dtype = resolve_kv_dtype(kv_dtype)
        if kv_dtype == "fp8" and not (self.kv_fp8_supported and self.cfg.head_dim == 128 and not self.rope_neox):
            raise ValueError(f"kv_dtype='fp8' needs the transformer backbone with head_dim 128 "
                             f"({type(self).__name__}, head_dim {self.cfg.head_dim})")
        weight_dtype = resolve_weight_dtype(weight_dtype)
        if weight_dtype == "fp8":
            if not (self.w_fp8_supported and self.small_batch_path):
                raise ValueError(f"weight_dtype='fp8' needs the transformer backbone's small-batch decode path "
                                 f"({type(self).__name__})")
            if batch_size > 8 or self.cfg.d_model != 2048:
                raise ValueError(f"weight_dtype='fp8' runs on the small-batch decode path only: batch_size <= 8 and "
                                 f"d_model 2048 (batch_size {batch_size}, d_model {self.cfg.d_model})")
            if kv_dtype == "fp8":
                raise ValueError("weight_dtype='fp8' cannot be combined with kv_dtype='fp8' (the FP8 KV cache runs "
                                 "the seven-launch sequence)")
        self._fp8 = kv_dtype == "fp8"
        self._w8 = weight_dtype == "fp8"
        _lib.require_gpu(prefix_conditioning, "prefix_conditioning")
        if prefix_conditioning.dim() != 3 or prefix_conditioning.shape[2] != self.cfg.d_model:
            # zk_prefill copies rows of Lc * d_model bf16: a wrong width would read out of bounds
            raise ValueError(f"prefix_conditioning must be [2B, Lc, {self.cfg.d_model}], "
                             f"got {tuple(prefix_conditioning.shape)}")
        spd = dict(top_p=0, top_k=0, min_p=0, linear=0.55, conf=0.4, quad=0.0, repetition_penalty=3.0,
                   repetition_penalty_window=2, temperature=1.0)
        spd.update(sampling_params or {})
        check_sampling_params(spd)
        c = self.cfg
        B = batch_size
        R = 2 * B
        P = 0 if audio_prefix_codes is None else int(audio_prefix_codes.shape[2])
        Lc = int(prefix_conditioning.shape[1])
        if self._w8:
            self.quantize_weights_fp8()
        live = getattr(self, "_streaming", None)
        live = live() if live is not None else None
        if live is not None:                # a stream() left unfinished works in the buffers this call takes over
            self._streaming = None
            live.close()
        row_off = getattr(rows, "row_off", None)        # a ragged request batch (plan_requests)
        ws = self._alloc(B, Lc, P, max_new_tokens, ragged=row_off is not None)
        # each row's context offset Lc_b - Lc, on the device for the whole generation (the captured step reads it)
        ws["row_off"] = None if row_off is None else torch.tensor(row_off, dtype=torch.int32, device=self.device)
        stream = _lib.stream_ptr(self.device)
        T, Ld, S = ws["T"], ws["Ld"], ws["S_pre"]
        D = c.d_model

        # codes -> delayed codes on device (model.py:288-295)
        codes = torch.full((B, N_CB, T), UNKNOWN, dtype=torch.int64, device=self.device)
        if audio_prefix_codes is not None:
            codes[..., :P] = audio_prefix_codes.to(self.device)
        if rows is not None:                # per-request budgets: nothing to write past P + n_b
            zrequests.budget_mask(codes, P, rows.budgets)
        call("zk_delay_apply", ptr(codes), B, N_CB, T, MASK, ptr(ws["delayed"]), stream)

        sp = SamplingParams(float(spd["temperature"]), float(spd["top_p"]), float(spd["min_p"]),
                            float(spd["linear"]), float(spd["conf"]), float(spd["quad"]), int(spd["top_k"]),
                            int(spd["repetition_penalty_window"]), float(cfg_scale), int(force_full_length))
        gen = None
        if noise == "torch":
            if row_base:
                raise ValueError("noise='torch' is one process's stream (row_base must be 0)")
            gen = generator if generator is not None else \
                torch.cuda.default_generators[_lib.device_index(self.device)]
            seed, off0 = int(gen.initial_seed()), int(gen.get_offset())
            stride, incr = zsampling.torch_noise_policy(B * N_CB * VOCAB, self.device)
            st = self._gen_state(ws, B, seed, 0, (1, off0, stride, incr))
        elif noise == "keyed":
            st = self._gen_state(ws, B, seed, row_base)
        else:
            raise ValueError(f"noise must be 'keyed' or 'torch', not {noise!r}")
        # a request batch: the device zk_row_params [B] the rows-mode sampler reads (None: the batch-wide one)
        ws["rows"] = None
        if rows is not None:
            if noise != "keyed":
                raise ValueError("a request batch samples from the keyed noise only")
            ws["rows"] = torch.frombuffer(bytearray(bytes(zrequests.row_params(rows))),
                                          dtype=torch.uint8).to(self.device)
        ws["scal"].zero_()

        # ---- prefill (model.py:297-319, _prefill 181-202)
        if self.c_step:        # the same sequence enqueued by the C ABI
            condb = ws["cond_keep"] = prefix_conditioning.to(torch.bfloat16).contiguous()   # alive until copied
            self._c_prefill(ws, B, st, sp, condb, Lc, P, stream)
        else:
            x = ws["x"][: R * S].view(R, S, D)
            x[:, :Lc].copy_(prefix_conditioning.to(torch.bfloat16))
            if ws["row_off"] is not None:   # frames at Lc_b ...; the positions behind a row's own S_b hold zeros
                x[:, Lc:].fill_(pad_fill)
                call("zk_embed_codes_rows", ptr(ws["delayed"]), B, P + 1, N_CB, Ld * N_CB, Ld, ptr(self.emb), VOCAB,
                     D, 2, ptr(ws["x"]), S, Lc, ptr(ws["row_off"]), stream)
            else:
                call("zk_embed_codes", ptr(ws["delayed"]), B, P + 1, N_CB, Ld * N_CB, Ld, None, 0, ptr(self.emb),
                     VOCAB, D, 2, ptr(ws["x"]), S, Lc, None, None, c.eps, None, None, stream)
            L0 = self.layers[0]
            if self.embed_norm:
                call("zk_layernorm", ptr(ws["x"]), ptr(L0["ln1_w"]), ptr(L0["ln1_b"]), c.eps, R * S, D,
                     ptr(ws["xn"]), stream)
            else:
                self._prenorm(ws, R * S, stream, None)
            self._layers(ws, R * S, R, S, True, stream, None)
            self._heads(ws, R, S, stream, None)
            self._sample(ws, ws["part"], ws["splits"]["heads"], st, sp, 1, P + 1, stream)
        if _after_prefill is not None:      # test hook (teacher forcing of the first frame)
            _after_prefill(ws["delayed"][..., P + 1:P + 2])
        # Debug logging. The sampler statistics need the logits of every step (one step per poll);
        # model.py:381's EOS message on the root logger only needs the steps where a row entered EOS
        # mode, which are recovered at poll boundaries from the eos_mode / steps_after words
        # (`_log_new_eos`), so a root logger at DEBUG level keeps multi-step polls (<= 6 steps, the
        # EOS hold-off, so the detection offset is exact).
        logdbg = zsampling.debug_enabled()
        eosdbg = not logdbg and logging.getLogger().isEnabledFor(logging.DEBUG)
        if zsampling.debug_enabled():       # the reference's sampler statistics (sampling.py:287-322)
            zsampling.log_sampling_stats(
                zsampling.engine_logits_row(ws["dbg"][0, 0], True, False, EOS, force_full_length), spd, None, 1.0, EOS)
        if trace is not None:
            trace.setdefault("logits", []).append(ws["dbg"].clone())
            trace.setdefault("tokens", []).append(ws["tok0"].view(B, N_CB, 1).long().clone())

        # ---- state for the loop (model.py:316-342)
        max_steps = Ld - (P + 1)
        ws["scal"].copy_(torch.tensor([P + 2, S, 1, 0, 0, max_steps] + [0] * 10, dtype=torch.int32))
        ws["eos_mode"].zero_()
        ws["steps_after"].fill_(6)
        ws["remaining"].fill_(max_steps)
        ws["stopping"].zero_()
        ws["act"].zero_()
        ws["rp"].fill_(float(spd["repetition_penalty"]))
        if rows is not None:                # per request: remaining = n_b + 9 - 1 (model.py:335), its own penalty
            ws["remaining"].copy_(torch.tensor([n + N_CB - 1 for n in rows.budgets], dtype=torch.int32))
            ws["rp"].copy_(torch.tensor([float(p["repetition_penalty"]) for p in rows.params]))
            pad_rows = rows.pad
        if pad_rows:                        # padding rows: out of the EOS protocol (docstring)
            ws["eos_mode"][B - pad_rows:] = 1
            ws["steps_after"][B - pad_rows:] = 0
            ws["remaining"][B - pad_rows:] = 0

        # ---- decode loop (model.py:345-432)
        per_poll = 1 if (callback is not None or trace is not None or logdbg) else max(1, poll_every)
        if eosdbg:
            per_poll = min(per_poll, 6)
            eos_prev = ws["eos_mode"].cpu()
        graph = None
        # steps per graph replay: a replay boundary leaves the GPU idle for 11-13 us (rocprofv3 kernel
        # trace, profiles/r5_trace_gaps_c{2,3}.txt: the gap before every step's first kernel), a kernel
        # boundary inside the graph ~1 us. G divides the poll length; the steps after the last one are
        # no-ops (every kernel tests the done word), so the final poll may run up to G - 1 of them
        G = max(g for g in range(1, min(self.graph_steps, per_poll) + 1) if per_poll % g == 0)
        if use_graph and trace is None:
            graph = self._capture(ws, B, st, sp, stream, G)
        return SimpleNamespace(ws=ws, B=B, P=P, st=st, sp=sp, spd=spd, stream=stream, gen=gen,
                               off0=off0 if gen is not None else 0, incr=incr if gen is not None else 0,
                               force_full_length=force_full_length, callback=callback, progress=progress, trace=trace,
                               logdbg=logdbg, eosdbg=eosdbg, eos_prev=eos_prev if eosdbg else None, per_poll=per_poll,
                               G=G, graph=graph, max_steps=max_steps, streamer=None, result=None, finished=False,
                               rows=rows)

    def _finish(self, run) -> torch.Tensor:
        """The end of a generation, run to its end or left early: waits for what is enqueued and advances the
        torch-noise generator by the sampler calls that were made. Returns the step words."""
        if run.streamer is not None:
            run.streamer.drain()
        scal = run.ws["scal"].cpu()
        if not run.finished and run.gen is not None and float(run.spd["temperature"]) > 0:
            # sampler calls the reference made: the prefill sample, one per loop iteration
            # (scal[2] counts from 1) and one per EOS resample (scal[4]); greedy draws nothing
            run.gen.set_offset(run.off0 + (int(scal[2]) + int(scal[4])) * run.incr)
        run.finished = True
        return scal

    @torch.inference_mode()
    def _decode_loop(self, run):
        """generate()'s decode loop (model.py:345-432) and output trim; leaves the codes in run.result. With a
        streamer (stream()) it is a generator of StreamChunk: the windows a poll made ready are decoded after the
        next poll has been launched. Without one it yields nothing and enqueues what generate() always has."""
        ws, B, P, st, sp, spd, stream = run.ws, run.B, run.P, run.st, run.sp, run.spd, run.stream
        callback, progress, trace, logdbg, eosdbg = run.callback, run.progress, run.trace, run.logdbg, run.eosdbg
        per_poll, G, graph, max_steps, eos_prev, sm = run.per_poll, run.G, run.graph, run.max_steps, run.eos_prev, run.streamer
        done_steps = 0
        pending = None                      # stream(): the windows the last poll made ready
        try:
            while True:
                n = min(per_poll, max_steps - done_steps)
                if n <= 0:
                    break
                if logdbg:                      # state the step starts from (debug logging only)
                    pre = (ws["scal"].cpu(), ws["act"][0].item(), ws["rp"][0].item(), ws["eos_mode"].cpu())
                if graph is not None:
                    call("zk_graph_launch", graph, -(-n // G), stream)
                else:
                    for _ in range(n):
                        self._decode_step(ws, B, st, sp, stream)
                done_steps += n
                if sm is not None:
                    ev = sm.mark()
                    if pending is not None:     # behind this poll's launch: the decode steps do not wait for the DAC
                        yield from sm.emit(ws["delayed"], pending)
                if logdbg:
                    self._log_step(ws, spd, pre, run.force_full_length)
                if trace is not None:
                    trace["logits"].append(ws["dbg"].clone())
                scal = ws["scal"].cpu()
                if eosdbg:
                    eos_prev = self._log_new_eos(ws, eos_prev, int(scal[0]) - 1)
                if progress is not None:
                    progress.update(n)
                if callback is not None:
                    off = int(scal[0]) - 1
                    frame = ws["delayed"][..., off:off + 1]
                    if not callback(frame, done_steps, max_steps):
                        break
                if trace is not None:
                    off = int(scal[0]) - 1
                    trace["tokens"].append(ws["delayed"][..., off:off + 1].clone())
                if sm is not None:              # frames < off - 9 are final: the count finalize() trims to
                    pending = sm.plan(P, int(scal[0]) - 1 - N_CB, False, done_steps, ev)
                if int(scal[3]):
                    break
            scal = self._finish(run)
            offset = int(scal[0]) - 1
            if trace is not None:
                trace["delayed"] = ws["delayed"].clone()
                trace["offset"] = offset
            if sm is not None:                  # what the last poll made ready, then every remaining frame
                if pending is not None:
                    yield from sm.emit(ws["delayed"], dict(pending, ev=None))
                yield from sm.emit(ws["delayed"], sm.plan(P, offset - N_CB, True, done_steps, None))
                sm.drain()
            if run.rows is not None:            # per-request trim; the padding requests' codes are dropped
                run.result = zrequests.trim_request_codes(ws["delayed"], P, run.rows.budgets,
                                                          offset)[:run.rows.real]
            else:
                run.result = finalize(ws["delayed"], offset, P, stream)
        except GeneratorExit:                   # the consumer left early: drain, leave torch's generator right
            self._finish(run)
            raise

    def _log_new_eos(self, ws, eos_prev, off_last):
        """model.py:381's message for the rows that entered EOS mode during the last poll.
        A row detected at offset o has had its hold-off counter (6 at detection, model.py:384)
        decremented once per later step (model.py:360-362), so o = off_last - 6 + steps_after
        while the poll is at most 6 steps long."""
        eos1 = ws["eos_mode"].cpu()
        new = ((eos1 != 0) & (eos_prev == 0)).nonzero(as_tuple=True)[0].tolist()
        if new:
            sa = ws["steps_after"].cpu()
            by_off = {}
            for r in new:
                by_off.setdefault(off_last - 6 + int(sa[r]), []).append(r)
            for off in sorted(by_off):
                logging.debug(f"Detected EOS in codebook 0 for samples: {by_off[off]} at offset {off}. "
                              "Resampling with -torch.inf.")
        return eos1

    def _log_step(self, ws, spd, pre, force_full_length):
        """Debug logging of one executed decode step (per_poll = 1): the sampler statistics of
        utterance 0 / codebook 0 on the zonos.sampling loggers and model.py:381's EOS message."""
        scal0, act0, rp0, eos0 = pre
        off = int(scal0[0])                 # the reference's `offset` of this step
        if int(scal0[3]):
            return                          # generation had finished: the step was a no-op
        scal1 = ws["scal"].cpu()
        resampled = int(scal1[4]) > int(scal0[4])
        if resampled:
            eos1 = ws["eos_mode"].cpu()
            rows = ((eos1 != 0) & (eos0 == 0)).nonzero(as_tuple=True)[0].tolist()
            logging.debug(f"Detected EOS in codebook 0 for samples: {rows} at offset {off}. "
                          "Resampling with -torch.inf.")
        if not zsampling.debug_enabled():
            return
        x = zsampling.engine_logits_row(ws["dbg"][0, 0], False, bool(act0), EOS, force_full_length)
        gen = ws["delayed"][0, 0, :off]
        zsampling.log_sampling_stats(x, spd, gen, rp0, EOS)
        if resampled:                       # the second sample_from_logits call (model.py:388)
            if int(ws["eos_mode"][0].item()) and not int(eos0[0]):
                x[EOS] = -math.inf
            zsampling.log_sampling_stats(x, spd, gen, rp0, EOS)

    def last_logits(self) -> torch.Tensor:
        """fp32 CFG logits (before bias) of the last executed step [B][9][1026] (test hook)."""
        return self._ws["dbg"]

    def last_tokens(self) -> torch.Tensor:
        """Sampled tokens (first draw) of the last executed step, int32 [B][9] (test hook; the
        frame may hold the delay pattern's MASK or a prefix code instead, model.py:305-306)."""
        return self._ws["tok0"].view(-1, N_CB)

    def _capture(self, ws, B, st, sp, stream, steps: int = 1):
        if ws.get("graph"):
            call("zk_graph_destroy", ws["graph"])
            ws["graph"] = None
        # capture on a side stream (torch's default stream cannot be captured)
        s = torch.cuda.Stream(self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        sp_ = s.cuda_stream
        call("zk_graph_begin", sp_)
        try:
            for _ in range(steps):
                self._decode_step(ws, B, st, sp, sp_)
        finally:
            g = _lib.P()
            call("zk_graph_end", sp_, C.byref(g))
        torch.cuda.current_stream(self.device).wait_stream(s)
        ws["graph"] = g.value
        ws["_keep"] = (st, sp)
        return g.value


def finalize(delayed: torch.Tensor, offset: int, P: int, stream) -> list:
    """Output trim (model.py:437-457), on the device."""
    B, K, Ld = delayed.shape
    out = torch.empty(B, K, Ld - K, dtype=torch.int64, device=delayed.device)
    call("zk_delay_revert", ptr(delayed), B, K, Ld, ptr(out), stream)
    eos_pos = (out[:, 0, :] == EOS).int().argmax(dim=-1)
    eos_pos[eos_pos == 0] = out.shape[2]
    out = out[..., : offset - 9]
    out.masked_fill_(out >= 1024, 0)
    eos_pos = eos_pos.tolist()
    return [out[i, :, P:eos_pos[i]].clone() for i in range(out.shape[0])]
