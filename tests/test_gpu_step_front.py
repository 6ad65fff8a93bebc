"""GPU: the decode launches whose argument order was arranged for the kernel-argument preload (k_gemm_ws
behind zk_gemm_bf16, k_resid_ln_d2k512 behind zk_resid_ln; DESIGN §6 "Kernel-argument preload"), at their
smallest shapes, each launched twice: with the step word clear the result is the op's oracle result (the
references and tolerances of test_gpu_ops.py's tests of the same entries), with it set every output buffer,
pre-filled with a sentinel, comes back bit-unchanged. Inputs and outputs live inside larger tensors with
slack on both sides, and the slack must stay untouched too."""
import pytest
import torch
import torch.nn.functional as F

DEV = "cuda"
pytestmark = pytest.mark.gpu
SLACK = 128 * 128          # elements on each side of every buffer
SENTINEL = 1234.5


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from zonos_amd import _lib
    _lib.load()


def _inside(t):
    """A copy of t placed in the middle of a larger tensor (the view is contiguous)."""
    big = torch.full((t.numel() + 2 * SLACK,), SENTINEL, dtype=t.dtype, device=DEV)
    v = big[SLACK:SLACK + t.numel()].view(t.shape)
    v.copy_(t)
    return big, v


def _sentinel(shape, dtype):
    big = torch.full((2 * SLACK + int(torch.Size(shape).numel()),), SENTINEL, dtype=dtype, device=DEV)
    return big, big[SLACK:big.numel() - SLACK].view(shape)


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _untouched(big, inner_too):
    ref = torch.full_like(big, SENTINEL)
    if inner_too:
        return torch.equal(_bits(big), _bits(ref))
    return torch.equal(_bits(big[:SLACK]), _bits(ref[:SLACK])) and torch.equal(_bits(big[-SLACK:]), _bits(ref[-SLACK:]))


def _word(v):
    return torch.full((1,), v, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("M,N,K,nsplit", [(17, 64, 128, 1), (17, 64, 256, 2), (128, 48, 128, 1), (128, 48, 256, 2)])
def test_gemm_slabs_front(M, N, K, nsplit):
    from zonos_amd._lib import call, ptr, stream_ptr
    from zonos_amd.engine import pack_weights
    g = torch.Generator(device="cpu").manual_seed(M + N + K)
    A = torch.randn(M, K, generator=g).to(torch.bfloat16)
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16).to(DEV)
    _, A_d = _inside(A.to(DEV))
    s = stream_ptr()
    Wpk = pack_weights(W, s)
    ref = A.to(DEV).float() @ W.float().t()
    for skip in (0, 1):
        big, part = _sentinel((nsplit, M, N), torch.float32)
        word = _word(skip)
        call("zk_gemm_bf16", ptr(A_d), K, ptr(Wpk), M, N, K, nsplit, 0, ptr(part), None, ptr(word), s)
        torch.cuda.synchronize()
        assert _untouched(big, inner_too=bool(skip))
        if not skip:
            got = part.sum(0)
            # test_gpu_ops.test_gemm_vs_fp32: fp32 accumulation of bf16 products
            assert torch.allclose(got, ref, atol=2e-3 * (K / 2048) ** 0.5, rtol=1e-3), (got - ref).abs().max()


@pytest.mark.parametrize("M,Fd,D", [(17, 32, 256), (128, 24, 256)])
def test_gemm_swiglu_front(M, Fd, D):
    from zonos_amd._lib import call, ptr, stream_ptr
    from zonos_amd.engine import pack_weights
    g = torch.Generator(device="cpu").manual_seed(1)
    A = torch.randn(M, D, generator=g).to(torch.bfloat16)
    W1 = (torch.randn(2 * Fd, D, generator=g) / D ** 0.5).to(torch.bfloat16)
    ref_y, ref_g = F.linear(A, W1).chunk(2, dim=-1)          # bf16 CPU like the reference
    ref = ref_y * F.silu(ref_g)
    s = stream_ptr()
    Wp = torch.empty_like(W1).to(DEV)
    call("zk_permute_fc1", ptr(W1.to(DEV)), Fd, D, ptr(Wp), s)
    Wp = pack_weights(Wp, s)
    _, A_d = _inside(A.to(DEV))
    for skip in (0, 1):
        big, out = _sentinel((M, Fd), torch.bfloat16)
        word = _word(skip)
        call("zk_gemm_bf16", ptr(A_d), D, ptr(Wp), M, 2 * Fd, D, 1, 1, None, ptr(out), ptr(word), s)
        torch.cuda.synchronize()
        assert _untouched(big, inner_too=bool(skip))
        if not skip:
            err = (out.float().cpu() - ref.float()).abs()
            # test_gpu_ops.test_gemm_swiglu: one bf16 ulp of the product plus accumulation-order flips
            assert err.max() < 0.05 and (err > 0).float().mean() < 0.05, err.max()


@pytest.mark.parametrize("nsplit", [4, 8])
def test_resid_ln_front(nsplit):
    from zonos_amd._lib import call, ptr, stream_ptr
    rows, D = 2, 2048
    g = torch.Generator(device="cpu").manual_seed(nsplit)
    x = torch.randn(rows, D, generator=g).to(torch.bfloat16)
    w = (1 + 0.1 * torch.randn(D, generator=g)).to(torch.bfloat16)
    b = (0.1 * torch.randn(D, generator=g)).to(torch.bfloat16)
    part = torch.randn(nsplit, rows, D, generator=g)
    ref_x = x + part.sum(0).to(torch.bfloat16)
    ref_xn = F.layer_norm(ref_x, (D,), w, b, 1e-5)
    (_, xd), (_, wd), (_, bd), (_, pd) = (_inside(t.to(DEV)) for t in (x, w, b, part))
    s = stream_ptr()
    for skip in (0, 1):
        bo, xo = _sentinel((rows, D), torch.bfloat16)
        bn, xn = _sentinel((rows, D), torch.bfloat16)
        word = _word(skip)
        call("zk_resid_ln", ptr(pd), nsplit, ptr(xd), ptr(wd), ptr(bd), 1e-5, rows, D, ptr(xo), ptr(xn), 0, ptr(word), s)
        torch.cuda.synchronize()
        assert _untouched(bo, inner_too=bool(skip)) and _untouched(bn, inner_too=bool(skip))
        if not skip:
            # test_gpu_ops.test_layernorm_and_resid_ln
            assert (xo.float().cpu() - ref_x.float()).abs().max() < 0.07
            assert (xn.float().cpu() - ref_xn.float()).abs().max() < 0.06
