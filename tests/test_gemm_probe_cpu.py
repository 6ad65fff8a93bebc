"""CPU: the GEMM probe (tests/gemm_probe.py) itself. Its inputs have the properties it claims, the clean fp32
restatement meets the exact criterion, every mutant fails it on every case aimed at it, the old Gaussian
assertion is shown to miss what the probe sees, and the case table of tests/test_gpu_gemm_probe.py runs the
kernel instantiations it claims (by the library's host-only plan queries)."""
import os

import numpy as np
import pytest
import torch

from tests import gemm_probe as P

IDS = [c.name for c in P.CASES]


def _setup(case, which=0):
    d = P.make_data(case, which)
    return d, P.reference(case, d), P.make_a(case, d), P.pack_weights(d.W)


def _fails(case, exp, out):
    try:
        P.compare(case, exp, P.inside(case, out))
        P.check_guards(case, out)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("case", P.CASES, ids=IDS)
def test_properties_clean_and_mutants(case):
    """Per case: check_properties() on both data sets; the clean emulate() is exact with intact guards; each
    mutant aimed at the case fails. A skip case: the word 1 leaves every word of the buffer as it was."""
    d, exp, a_buf, packed = _setup(case)
    P.check_properties(case, d, exp)
    d1 = P.make_data(case, 1)
    P.check_properties(case, d1, P.reference(case, d1))
    assert (d1.W != d.W).any(axis=1).all() and (d1.A != d.A).any()
    out = P.make_out(case, d)
    if case.skip:
        before = out.clone()
        P.emulate(case, d, a_buf, packed, out, skip_word=1)
        assert torch.equal(out, before)
        for mutant in ("skip_ignored", "skip_partial"):
            o = P.make_out(case, d)
            P.emulate(case, d, a_buf, packed, o, skip_word=1, mutant=mutant)
            assert not torch.equal(o, before), mutant
    P.emulate(case, d, a_buf, packed, out)
    res = P.compare(case, exp, P.inside(case, out))
    P.check_guards(case, out)
    assert res["flips"] <= res["permitted"]
    for mutant in P.MUTANTS:
        if P.mutant_applies(mutant, case) and not case.skip:
            o = P.make_out(case, d)
            P.emulate(case, d, a_buf, packed, o, mutant=mutant)
            assert _fails(case, exp, o), f"{mutant} passes on {case.name}"


def test_every_mutant_has_cases():
    for mutant in P.MUTANTS:
        n = sum(P.mutant_applies(mutant, c) for c in P.CASES)
        assert n >= 3, (mutant, n)


def test_second_data_set_in_the_same_buffers():
    """A result left over from the first data set does not pass for the second."""
    firsts = {}
    for c in P.CASES:
        firsts.setdefault((c.entry, c.mode, c.nsplit > 1), c)
    assert len(firsts) >= 6
    for case in firsts.values():
        d0, e0, a0, p0 = _setup(case, 0)
        d1, e1, _, _ = _setup(case, 1)
        out = P.make_out(case, d0)
        P.emulate(case, d0, a0, p0, out)
        P.compare(case, e0, P.inside(case, out))
        assert _fails(case, e1, out)


def test_pack_weights_layout():
    W = np.arange(80 * 64, dtype=np.int32).reshape(80, 64)
    pk = P.pack_weights(W)
    assert pk.shape == (8, 2, 64, 8)
    # lane 16 kq + nl of fragment (nt, kc) holds W[16 nt + nl][32 kc + 8 kq .. + 8] (k_pack_w, gemm.hip)
    for nt, kc, lane in ((0, 0, 0), (1, 1, 17), (4, 0, 63), (4, 1, 35)):
        n, k = nt * 16 + (lane & 15), kc * 32 + (lane >> 4) * 8
        assert (pk[nt, kc, lane] == W[n, k:k + 8]).all()
    assert (pk[5:] == 0).all()
    assert (P.unpack_weights(pk)[:80] == W).all()


def test_case_table_runs_the_claimed_instantiations():
    from zonos_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    seen, seen_ln = set(), set()
    for c in P.CASES:
        if c.entry == "gemm":
            p = _lib.gemm_plan(c.M, c.N, c.K, c.nsplit, c.mode)
        else:
            p = _lib.gemv_plan(c.M, c.N, c.K, c.mode, c.ln)
        for k, v in c.want:
            assert p[k] == v, (c.name, k, v, p)
        for entry, mode, want in P.REQUIRED:
            if entry == c.entry and mode == c.mode and all(p[k] == v for k, v in want):
                seen.add((entry, mode, want))
        if c.ln:
            seen_ln.update((m, w) for m, w in P.REQUIRED_LN if m == c.mode and all(p[k] == v for k, v in w))
    assert not set(P.REQUIRED) - seen, sorted(set(P.REQUIRED) - seen)
    assert not set(P.REQUIRED_LN) - seen_ln, sorted(set(P.REQUIRED_LN) - seen_ln)
    # the N forms of the k_gemm_ws slab stores, per workgroup width: N % 4 == 0 with a partial last workgroup,
    # N % 4 != 0, a 16-column tile wholly past N; the skip word and a strided A in every family
    for ncw in (2, 3, 4, 5):
        ws = [c for c in P.CASES if c.entry == "gemm" and c.mode == 0 and ("ncw", ncw) in c.want]
        assert any(c.N % 4 == 0 and c.N % (16 * ncw) for c in ws) and any(c.N % 4 for c in ws), ncw
        assert any(-(-c.N // 16) % ncw for c in ws), ncw
    # zk_gemv_fused: both row counts of each LDS image (M 1 and 2, M 3 and 16) in every mode, with and without the
    # prologue, and each of them at more than one N
    for mode in (0, 1, 2):
        for ln in (False, True):
            for xr, Ms in ((2, {1, 2}), (16, {3, 16})):
                got = {c.M for c in P.CASES if c.entry == "gemv" and (c.mode, c.ln) == (mode, ln)
                       and ("xr", xr) in c.want and not c.skip}
                assert Ms <= got, (mode, ln, xr, got)
    for M in (1, 2, 3, 16):
        assert len({c.N for c in P.CASES if c.entry == "gemv" and c.M == M}) >= 4, M
    for sel in (lambda c: c.skip, lambda c: c.row_stride != c.K):
        fam = {dict(c.want).get("family", "gemv") for c in P.CASES if sel(c)}
        assert fam == {"rk", "ws", "tile", "pf", "gemv"}, fam


def test_old_assertion_misses_what_the_probe_sees(capsys):
    """The i.i.d. Gaussian data and the assertion of test_gemm_vs_fp32 (tests/test_gpu_ops.py), on the CPU: of a few
    hundred single-product drops a good share passes it, and a row stride ignored or a clamped row stored cannot fail
    it at all (it has lda = K and nothing around its output; it passes no skip word either, so an ignored word is
    never exercised). The figures are printed (profiles/gemm_probe_tests.txt records them)."""
    lines = []
    for K in (2048, 8192):
        M, N = 16, 64
        g = torch.Generator().manual_seed(K)
        A = torch.randn(M, K, generator=g).to(torch.bfloat16).float()
        W = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16).float()
        ref = A @ W.t()
        atol = 2e-3 * (K / 2048) ** 0.5
        passed, trials = 0, 400
        for i in range(trials):
            m, n, k = i % M, (7 * i) % N, (131 * i + 17) % K
            got = ref.clone()
            got[m, n] -= A[m, k] * W[n, k]                      # one product dropped
            passed += bool(torch.allclose(got, ref, atol=atol, rtol=1e-3))
        lines.append(f"K={K}: the old assertion passes {passed} of {trials} single-product drops")
        assert passed >= trials // 20          # (a demonstration; measured 26 % / 55 %)
        # the same drops on the probe's data: every one changes an integer
        case = P.Case("gemm", M, N, K)
        d = P.make_data(case, 0)
        exp = P.reference(case, d)
        for i in range(trials):
            m, n, k = i % M, (7 * i) % N, (131 * i + 17) % K
            assert int(d.A[m, k]) * int(d.W[n, k]) != 0
        bits = P._bits(exp.slabs, torch.float32).copy()
        dropped = exp.slabs.copy()
        dropped[0, 3, 5] -= int(d.A[3, 9]) * int(d.W[5, 9])
        with pytest.raises(AssertionError):
            P.compare(case, exp, P._bits(dropped, torch.float32))
        P.compare(case, exp, bits)
    # what the old test cannot see by construction: with lda = K a stride that is ignored reads the same elements, and
    # a row M - 1 also stored to row M changes nothing the assertion looks at
    case = P.Case("gemm", 16, 64, 256)
    d, exp, a_buf, packed = _setup(case)
    ref = torch.from_numpy(d.A.astype(np.float32)) @ torch.from_numpy(d.W.astype(np.float32)).t()
    for mutant in ("lda_ignored", "row_clamp_stored"):
        out = P.make_out(case, d)
        P.emulate(case, d, a_buf, packed, out, mutant=mutant)
        got = torch.from_numpy(P.inside(case, out)).view(torch.float32).reshape(16, 64)
        assert torch.allclose(got, ref, atol=2e-3 * (256 / 2048) ** 0.5, rtol=1e-3)
        lines.append(f"{mutant}: passes the old assertion (lda = K, nothing around the output)")
    # ... and it passes no skip word, so a launch that ignores the word is never asked to skip (nothing to run)
    lines.append("skip_ignored: cannot fail the old test, which passes no skip word")
    with capsys.disabled():
        print("\n" + "\n".join(lines))
