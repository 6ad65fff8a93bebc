"""The GEMM / GEMV kernels (zonos_amd/csrc/gemm.hip, gemm_pf.hip) on the exact-integer cases of
tests/gemm_probe.py: every fp32 output and the residual epilogue bit-equal to the integer reference, the SwiGLU
epilogue bit-equal up to the permitted silu flips, NaN around A, guard bands around the outputs, a strided A, the
skip word, each case on two data sets in the same buffers and on the kernel instantiation it claims (asserted by
the library's plan query). tests/test_gemm_probe_cpu.py shows what these cases detect. The figures per kernel
family are printed when the module is done (pytest -s); profiles/gemm_probe_tests.txt records them."""
import collections

import numpy as np
import pytest
import torch

from . import gemm_probe as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
STATS = collections.defaultdict(lambda: dict(cases=0, exact=0, flips=0, permitted=0, ms=0.0))


@pytest.fixture(scope="module", autouse=True)
def _lib():
    """Loads the library; when the module's tests are over, prints their figures per kernel family and mode."""
    from zonos_amd import _lib
    _lib.load()
    yield
    for (family, mode), s in sorted(STATS.items()):
        print(f"\n{family} mode {mode}: {s['cases']} cases, {s['exact']} bit-exact elements, "
              f"{s['flips']} SwiGLU flips of {s['permitted']} permitted, {s['ms']:.2f} ms in the launches", end="")


def _plan(case):
    from zonos_amd import _lib
    if case.entry == "gemm":
        p = _lib.gemm_plan(case.M, case.N, case.K, case.nsplit, case.mode)
        return p, p["family"]
    return _lib.gemv_plan(case.M, case.N, case.K, case.mode, case.ln), "gemv_f"


def _launch(case, bufs, skip):
    from zonos_amd._lib import call, ptr, stream_ptr
    a = ptr(bufs["a"]) + 2 * case.a_off
    out = ptr(bufs["out"]) + P.guard_len(case) * bufs["out"].element_size()
    s = stream_ptr()
    if case.entry == "gemm":
        call("zk_gemm_bf16", a, case.row_stride, ptr(bufs["wpk"]), case.M, case.N, case.K, case.nsplit, case.mode,
             out if case.mode == 0 else None, out if case.mode else None, ptr(skip), s)
    else:
        lw, lb = (ptr(bufs["ln_w"]), ptr(bufs["ln_b"])) if case.ln else (None, None)
        call("zk_gemv_fused", a, case.row_stride, ptr(bufs["wpk"]), case.M, case.N, case.K, case.mode, lw, lb, 1e-5,
             out if case.mode == 0 else None, out if case.mode else None, ptr(skip), s)


def _load(case, d, bufs):
    """Data set d into the buffers of the case (allocated on first use, the same ones afterwards)."""
    from zonos_amd._lib import call, ptr, stream_ptr
    new = dict(a=P.make_a(case, d), w=P.weight_values(case, d).view(torch.int16), out=P.make_out(case, d))
    if case.ln:
        new["ln_w"], new["ln_b"] = P._bf16_bits(d.ln_w), P._bf16_bits(d.ln_b)
    for k, v in new.items():
        if k in bufs:
            bufs[k].copy_(v)
        else:
            bufs[k] = v.to(DEV)
    if "wpk" not in bufs:
        bufs["wpk"] = torch.empty((case.N + 63) // 64 * 64, case.K, dtype=torch.int16, device=DEV)
    call("zk_pack_weights", ptr(bufs["w"]), case.N, case.K, ptr(bufs["wpk"]), stream_ptr())
    if case.N * case.K <= 1 << 20:
        # the library's packing is the layout gemm_probe.emulate() reads
        want = P.pack_weights(new["w"].numpy())
        assert np.array_equal(bufs["wpk"].cpu().numpy().reshape(want.shape), want)


@pytest.mark.parametrize("case", P.CASES, ids=[c.name for c in P.CASES])
def test_exact(case):
    plan, family = _plan(case)
    for k, v in case.want:
        assert plan[k] == v, (case.name, k, v, plan)
    bufs = {}
    st = STATS[(family, case.mode)]
    st["cases"] += 1
    for which in (0, 1):
        d = P.make_data(case, which)
        exp = P.reference(case, d)
        _load(case, d, bufs)
        if case.skip:
            before = bufs["out"].clone()
            _launch(case, bufs, torch.ones(1, dtype=torch.int32, device=DEV))
            torch.cuda.synchronize()
            assert torch.equal(bufs["out"], before), f"{case.name}: a skipped launch wrote"
        skip = torch.zeros(1, dtype=torch.int32, device=DEV) if case.skip else None
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        _launch(case, bufs, skip)
        t1.record()
        torch.cuda.synchronize()
        res = P.compare(case, exp, P.inside(case, bufs["out"]))
        P.check_guards(case, bufs["out"])
        print(f"{case.name} set {which}: {family} {res} {t0.elapsed_time(t1):.3f} ms")
        for k in ("exact", "flips", "permitted"):
            st[k] += res[k]
        st["ms"] += t0.elapsed_time(t1)
