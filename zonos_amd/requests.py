"""Request batches: a batch whose utterances each carry their own sampling parameters, CFG scale, noise seed /
key and length budget, and whose rows are independent -- request b's codes are what ``generate()`` returns for
it at batch size 1 (``row_base = key``), whatever else shares the batch and whichever slot or rank it lands in.

``generate()`` keeps the reference's batch-wide protocol (one ``sampling_params`` / ``cfg_scale``, model.py:224-247;
every row redrawn when any row emits its first EOS, model.py:380-393). ``generate_requests()`` runs the same step
with the rows-mode sampler and EOS kernels (zk_sample_heads_rows / zk_eos_step_rows, DESIGN §6 "Request batches").
This module is the host side that needs no device: the request type, its validation, the per-row state the engine
uploads and the output trim."""
from __future__ import annotations

from dataclasses import dataclass
from types import SimpleNamespace

import torch

from . import _lib

EOS, MASK = 1024, 1025
N_CB = 9
# generate()'s sampling defaults (model.py:232-235)
DEFAULT_SAMPLING = dict(top_p=0, top_k=0, min_p=0, linear=0.55, conf=0.4, quad=0.0, repetition_penalty=3.0,
                        repetition_penalty_window=2, temperature=1.0)


@dataclass
class Request:
    """One utterance of a request batch. ``conditioning``: [2, Lc, D], its cond and uncond rows
    (``prepare_conditioning`` of one utterance). ``sampling_params`` is merged over generate()'s defaults.
    ``seed`` / ``key``: the keyed noise stream is (seed, step, draw, key, codebook, token) -- the request alone is
    ``generate(..., batch_size=1, seed=seed, row_base=key)``."""
    conditioning: torch.Tensor
    audio_prefix_codes: torch.Tensor | None = None    # [9, P] or [1, 9, P]
    max_new_tokens: int = 86 * 30
    cfg_scale: float = 2.0
    sampling_params: dict | None = None
    seed: int = 0
    key: int = 0
    force_full_length: bool = False


def _prefix(req: Request):
    p = req.audio_prefix_codes
    if p is None:
        return None
    if p.dim() == 3 and p.shape[0] == 1:
        p = p[0]
    if p.dim() != 2 or p.shape[0] != N_CB:
        raise ValueError(f"audio_prefix_codes must be [9, P] or [1, 9, P], got {tuple(req.audio_prefix_codes.shape)}")
    return p


def plan_requests(requests, d_model: int | None = None, pad: int = 0, ragged: bool = False) -> SimpleNamespace:
    """Validate a list of requests and lay out what the engine needs, without touching a device. Raises ValueError
    for an empty list, ragged prompts (conditionings of different Lc, prefixes of different P), cfg_scale == 1, a
    repetition window outside the sampler's, a malformed tensor or a budget below 1. ``pad``: the last ``pad``
    requests are padding (generate_sharded_requests' uniform shards): no budget, out of the EOS protocol.

    ``ragged=True`` accepts conditionings of different lengths (prefix lengths must still agree, and every Lc_b must
    be >= 1): ``Lc`` is then the longest, ``lcs`` the length of each request and ``row_off`` the int32 list [2B] of
    Lc_b - Lc <= 0, the cond rows and then the uncond rows as `stack_conditioning` orders them -- what the engine
    keeps on the device as each row's context offset (DESIGN §6 "Ragged request batches"). ``row_off`` is None when
    all lengths agree: the batch then takes the uniform path."""
    from .engine import check_sampling_params
    reqs = list(requests)
    if not reqs:
        raise ValueError("generate_requests needs at least one request (an empty list)")
    if not 0 <= pad < len(reqs):
        raise ValueError(f"pad={pad} must leave at least one real request of {len(reqs)}")
    params, prefixes = [], []
    for i, r in enumerate(reqs):
        c = r.conditioning
        if c.dim() != 3 or c.shape[0] != 2 or (d_model is not None and c.shape[2] != d_model):
            raise ValueError(f"request {i}: conditioning must be [2, Lc, {d_model or 'D'}] (the cond and uncond rows "
                             f"of one utterance), got {tuple(c.shape)}")
        if float(r.cfg_scale) == 1:
            raise ValueError(f"request {i}: cfg_scale == 1 is not supported (model.py:247)")
        if int(r.max_new_tokens) < 1:
            raise ValueError(f"request {i}: max_new_tokens={r.max_new_tokens} must be >= 1")
        spd = dict(DEFAULT_SAMPLING)
        spd.update(r.sampling_params or {})
        try:
            check_sampling_params(spd)
        except ValueError as e:
            raise ValueError(f"request {i}: {e}") from None
        params.append(spd)
        prefixes.append(_prefix(r))
    Lcs = {int(r.conditioning.shape[1]) for r in reqs}
    Ps = {0 if p is None else int(p.shape[1]) for p in prefixes}
    if len(Ps) > 1 or (len(Lcs) > 1 and not ragged):
        raise ValueError(f"ragged prompts are not supported: every request of a batch needs the same conditioning "
                         f"length and audio-prefix length (Lc in {sorted(Lcs)}, P in {sorted(Ps)}); "
                         f"generate_requests(..., ragged=True) takes conditionings of different lengths, "
                         f"audio prefixes of different lengths never")
    lcs = [int(r.conditioning.shape[1]) for r in reqs]
    Lc = max(lcs)
    row_off = None
    if len(Lcs) > 1:
        if min(lcs) < 1:
            raise ValueError(f"request {lcs.index(min(lcs))}: a ragged batch needs a conditioning of at least one "
                             f"token per request (Lc in {sorted(Lcs)})")
        row_off = [lc - Lc for lc in lcs] * 2
    real = len(reqs) - pad
    budgets = [int(r.max_new_tokens) if i < real else 0 for i, r in enumerate(reqs)]
    return SimpleNamespace(requests=reqs, params=params, prefixes=prefixes, Lc=Lc, P=Ps.pop(), budgets=budgets,
                           max_new=max(budgets), pad=pad, real=real, lcs=lcs, row_off=row_off)


def row_params(plan):
    """The zk_row_params [B] of a planned batch (ctypes; the engine uploads its bytes)."""
    arr = (_lib.RowParams * len(plan.requests))()
    for i, (r, spd) in enumerate(zip(plan.requests, plan.params)):
        arr[i] = _lib.RowParams(
            _lib.SamplingParams(float(spd["temperature"]), float(spd["top_p"]), float(spd["min_p"]),
                                float(spd["linear"]), float(spd["conf"]), float(spd["quad"]), int(spd["top_k"]),
                                int(spd["repetition_penalty_window"]), float(r.cfg_scale), int(r.force_full_length)),
            int(r.seed) & 0xFFFFFFFFFFFFFFFF, int(r.key), 0)
    return arr


def stack_conditioning(plan, pad_fill: float = 0.0) -> torch.Tensor:
    """[cond rows | uncond rows]: the [2B, Lc, D] layout of prepare_conditioning (model.py:213-218). A ragged plan
    pads every conditioning at the end to plan.Lc with zeros (``pad_fill``: the engine's test hook)."""
    cs = [r.conditioning for r in plan.requests]
    if plan.row_off is not None:
        cs = [torch.cat([c, c.new_full((2, plan.Lc - c.shape[1], c.shape[2]), pad_fill)], dim=1) for c in cs]
    return torch.cat([c[0:1] for c in cs] + [c[1:2] for c in cs])


def stack_prefixes(plan) -> torch.Tensor | None:
    return None if plan.P == 0 and plan.prefixes[0] is None else torch.stack(plan.prefixes)


def budget_mask(codes: torch.Tensor, P: int, budgets) -> torch.Tensor:
    """codes [B, 9, T] (before the delay pattern): request b's frames past its budget, t >= P + n_b, set to MASK --
    what the delay pattern of its own, shorter, generation holds there. The step only writes cells that hold -1
    (model.py:417-418), so a row whose budget is spent writes nothing and the frames it is fed from then on are
    the ones it would have been fed alone."""
    t = torch.arange(codes.shape[2], device=codes.device)
    n = torch.as_tensor(list(budgets), device=codes.device)
    codes.masked_fill_((t[None, :] >= (P + n)[:, None])[:, None, :], MASK)
    return codes


def trim_request_codes(delayed: torch.Tensor, P: int, budgets, offset: int | None = None) -> list:
    """The result of every request from the final delayed codes [B, 9, Ld] (plain tensors, any device): request b's
    is revert_delay(delayed[b])[:, P : min(P + n_b, first EOS of codebook 0)] with ids >= 1024 set to 0 -- what
    generate()'s output trim (model.py:437-457) gives the request alone. Frames at or past P + n_b never count,
    whatever the row wrote there while the rest of the batch ran on. ``offset`` (the final step offset of a loop
    that a callback ended early) keeps only the frames that are final, t < offset - 9."""
    B, K, Ld = delayed.shape
    T = Ld - K
    out = torch.stack([delayed[:, k, k + 1:k + 1 + T] for k in range(K)], dim=1)     # revert_delay_pattern
    res = []
    for b in range(B):
        end = min(P + int(budgets[b]), T)
        if offset is not None:
            end = min(end, max(P, offset - K))
        eos = (out[b, 0, :end] == EOS).nonzero()
        if eos.numel() and int(eos[0]) > 0:           # (generate() reads an EOS at frame 0 as "none")
            end = min(end, int(eos[0]))
        r = out[b, :, P:max(end, P)].clone()
        r.masked_fill_(r >= 1024, 0)
        res.append(r)
    return res
