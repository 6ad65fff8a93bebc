"""CPU: the C-ABI library builds/loads and exports every symbol include/zonos_hip.h declares;
host-side logic that needs no GPU."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "zonos_hip.h")


def header_symbols():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(zk_[a-z0-9_]+)\s*\(", txt)))


@pytest.fixture(scope="module")
def lib():
    from zonos_amd import build
    path = build.build()
    return ctypes.CDLL(path)


def test_library_exports_header(lib):
    syms = header_symbols()
    assert len(syms) >= 25
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in zonos_hip.h but not exported"


def test_python_binding_covers_header():
    from zonos_amd import _lib
    assert set(header_symbols()) == set(_lib.exported_symbols())


def test_version_and_error_without_gpu(lib):
    lib.zk_version.restype = ctypes.c_int
    assert lib.zk_version() >= 1
    lib.zk_last_error.restype = ctypes.c_char_p
    assert isinstance(lib.zk_last_error(), bytes)


def test_argument_validation_without_gpu(lib):
    # shape checks run on the host before any launch
    rc = lib.zk_gemm_bf16(None, ctypes.c_long(100), None, 0, 10, 64, 1, 0, None, None, None, None)
    assert rc != 0
    lib.zk_last_error.restype = ctypes.c_char_p
    assert b"zk_gemm_bf16" in lib.zk_last_error()


# the decode-attention entries' parameters, in ABI order (include/zonos_hip.h)
_DIMS = ["R", "H", "Hkv", "hd", "Smax", "ctx0", "ctx_dev", "work", "nsplit"]
_FUSED = ["part", "gemm_nsplit", "freqs"]
ATTN_DECODE_ENTRIES = {
    "zk_attn_decode": ["q", "k", "v", *_DIMS, "out", "skip", "stream"],
    "zk_attn_decode_qkv": [*_FUSED, "k", "v", *_DIMS, "out", "rope_neox", "skip", "stream"],
    "zk_attn_decode_qkv_sc": [*_FUSED, "k", "v", *_DIMS, "counters", "out", "rope_neox", "skip", "stream"],
    "zk_attn_decode_qkv_part": [*_FUSED, "k", "v", *_DIMS, "rope_neox", "skip", "stream"],
    "zk_attn_decode_f8": ["q", "k", "v", "k_scale", "v_scale", *_DIMS, "out", "skip", "stream"],
    "zk_attn_decode_qkv_f8": [*_FUSED, "k", "v", "k_scale", "v_scale", *_DIMS, "counters", "out", "skip", "stream"],
    "zk_attn_decode_q_part": ["q", "k", "v", *_DIMS, "skip", "stream"],
}


def test_attention_decode_entries_refuse_bad_arguments_without_gpu(lib):
    """Every decode-attention entry refuses, on the host and under its own name, a null K or V cache, a null
    output (where it writes one), null FP8 scales, head_dim 64, Smax 0 / 100, nsplit 0, nsplit > 1 without
    the work buffer and (fused forms) gemm_nsplit 0 / AT_MAXGS + 1. All other pointers are a dummy host
    buffer: nothing is launched, because a check fails first."""
    import ctypes as C
    src = open(os.path.join(REPO, "zonos_amd", "csrc", "attn_common.h")).read()
    maxgs = int(re.search(r"constexpr int AT_MAXGS = (\d+);", src).group(1))
    buf = C.create_string_buffer(64)
    lib.zk_last_error.restype = C.c_char_p
    ints = dict(R=2, H=4, Hkv=1, hd=128, Smax=256, ctx0=1, nsplit=2, gemm_nsplit=1, rope_neox=0)

    def refused(name, params, **bad):
        args = [bad[p] if p in bad else ints[p] if p in ints else None if p == "stream" else buf for p in params]
        rc = getattr(lib, name)(*[C.c_int(a) if isinstance(a, int) else a for a in args])
        err = lib.zk_last_error()
        assert rc != 0, (name, bad)
        assert err.startswith(name.encode() + b":"), (name, bad, err)
        assert b"launch failed" not in err, (name, bad, err)      # a check refused it, not the runtime

    for name, params in ATTN_DECODE_ENTRIES.items():
        cases = [dict(k=None), dict(v=None), dict(hd=64), dict(Smax=0), dict(Smax=100), dict(nsplit=0),
                 dict(nsplit=2, work=None)]
        cases += [dict(out=None)] if "out" in params else []
        cases += [dict(k_scale=None), dict(v_scale=None)] if "k_scale" in params else []
        cases += [dict(gemm_nsplit=0), dict(gemm_nsplit=maxgs + 1)] if "gemm_nsplit" in params else []
        for bad in cases:
            refused(name, params, **bad)
    # one split (no in-launch combine to do): still this entry's own checks and name
    refused("zk_attn_decode_qkv_sc", ATTN_DECODE_ENTRIES["zk_attn_decode_qkv_sc"], nsplit=1, hd=64)
    refused("zk_attn_decode_qkv_sc", ATTN_DECODE_ENTRIES["zk_attn_decode_qkv_sc"], nsplit=1, k=None)


def test_prefill_rejects_short_kv_cache_without_gpu(lib):
    """zk_prefill / zk_hybrid_prefill refuse a descriptor whose KV cache (smax keys) is shorter than
    the context of the last decode step (Lc + Ld), before any launch: the decode attention's context
    clamp is then only ever reached by no-op launches after the last step."""
    import ctypes as C

    from zonos_amd import _lib
    lays = (_lib.StepLayer * 1)()
    d = _lib.StepDesc()
    d.B, d.n_layer, d.d_model, d.smax, d.layers = 1, 1, 64, 256, C.cast(lays, C.c_void_p)
    d.st.Ld, d.st.K, d.st.V = 250, 9, 1026
    buf = C.create_string_buffer(16)
    lib.zk_last_error.restype = C.c_char_p
    assert lib.zk_prefill(C.byref(d), buf, 10, 0, buf, None) != 0      # 10 + 250 > 256
    assert b"KV cache" in lib.zk_last_error()


def test_gemm_warm_up_stays_inside_packed_image(lib):
    """The L2 warm-up a kernel issues for the next decode GEMM reads only tiles of that GEMM's packed
    weight image (the 48-column workgroups of the c5 Mamba in_proj -- N = 8512, 178 x 3 =
    534 tiles -- warmed 2 tiles past the 532-tile image). Every decode GEMM shape of c2-c5 at R = 128
    and R = 24, each split the engine may pick."""
    lib.zk_gemm_warm_tiles.restype = ctypes.c_int
    shapes = [(3072, 2048), (2048, 2048), (16384, 2048), (2048, 8192), (9234, 2048), (8512, 2048),
              (2048, 4096), (9280, 2048), (4400, 2048), (1000, 2048)]
    seen_narrow = False
    for M in (24, 72, 128):
        for N, K in shapes:
            for nsplit in (1, 2, 4, 8):
                if K % (nsplit * 64) or K // nsplit // 64 > 32:
                    continue
                for mode in (0, 1):
                    if mode == 1 and (nsplit != 1 or N % 16):
                        continue
                    t = lib.zk_gemm_warm_tiles(M, N, K, nsplit, mode, 2)
                    assert 0 <= t <= (N + 15) // 16, (M, N, K, nsplit, mode, t)
                    seen_narrow |= (N == 8512 and M == 128 and nsplit == 1 and t > 0)
    assert seen_narrow


def test_dac_conv_plan_of_product_and_test_shapes(lib):
    """zk_dac_conv_plan (the plan zk_dac_conv_cl / zk_dac_resunit_cl launch by) for the shapes the decoder, the
    encoder and the tests use: workgroup shape, FM, tile, window lead dx, window ring nx and LDS bytes, each
    evaluated by hand from the sizing rule of dac_cl.hip. Pair-shape workgroups are meant to fit two per CU
    (LDS <= 80 KiB); the 1x1 + residual convs at FM = 4 do not (84,992 B: their lead starts at its minimum, so
    the shrink loop never runs) and are listed by name below -- known, unmeasured, not to be fixed silently."""
    import ctypes as C
    lib.zk_dac_conv_plan.restype = C.c_int
    lib.zk_dac_conv_plan.argtypes = [C.c_int] * 10 + [C.POINTER(C.c_int32)]
    lib.zk_last_error.restype = C.c_char_p
    PAIR, FAT, F96, F192 = 0, 1, 2, 3
    B, T = 3, 1000

    def plan(Cin, Cout, ks, dil, Qn=T, nphase=1, resid=0, s_f32=0, fused=0):
        out = (C.c_int32 * 9)()
        rc = lib.zk_dac_conv_plan(fused, B, Cin, Cout, ks, dil, Qn, nphase, resid, s_f32, out)
        return rc, dict(zip(("shape", "fm", "tile", "dx", "nx", "lds", "nq", "tiles", "wg_per_cu"), out))

    rows = []       # (name, plan arguments, ks, (shape, FM, tile, dx, nx, LDS bytes))
    for c in (1536, 1024, 768, 512, 384, 256, 128):
        for dil, lds in ((1, 71680), (3, 74752), (9, 80896)):
            rows.append((f"k7 {c} dil {dil}", dict(Cin=c, Cout=c, ks=7, dil=dil), 7, (PAIR, 4, 128, 7, 3, lds)))
        rows.append((f"k3 {c}", dict(Cin=c, Cout=c, ks=3, dil=1), 3, (PAIR, 4, 128, 3, 3, 71680)))
        rows.append((f"convT {2 * c}->{c}", dict(Cin=2 * c, Cout=c, ks=2, dil=1, Qn=T + 1, nphase=4), 2,
                     (PAIR, 4, 128, 3, 3, 71680)))
        rows.append((f"1x1+res {c}", dict(Cin=c, Cout=c, ks=1, dil=1, resid=1), 1, (PAIR, 4, 128, 3, 5, 84992)))
    rows.append(("k7 1024->1536", dict(Cin=1024, Cout=1536, ks=7, dil=1), 7, (PAIR, 4, 128, 7, 3, 71680)))
    rows.append(("k7 64->128", dict(Cin=64, Cout=128, ks=7, dil=1), 7, (PAIR, 4, 128, 7, 3, 71680)))
    for c in (192, 96):
        rows.append((f"convT {2 * c}->{c}", dict(Cin=2 * c, Cout=c, ks=2, dil=1, Qn=T + 1, nphase=4 if c == 192 else 2), 2,
                     (PAIR, 3, 128, 3, 3, 60672)))
        for f32 in (0, 1):
            rows.append((f"1x1+res {c} f32={f32}", dict(Cin=c, Cout=c, ks=1, dil=1, resid=1, s_f32=f32), 1,
                         (PAIR, 3, 128, 3, 5, 73984)))
        for dil, lds in ((1, 134400), (3, 137472), (9, 143616)):
            rows.append((f"k7 {c} dil {dil}", dict(Cin=c, Cout=c, ks=7, dil=dil), 7, (FAT, 3, 512, 7, 3, lds)))
    rows.append(("1x1+res 64", dict(Cin=64, Cout=64, ks=1, dil=1, resid=1), 1, (PAIR, 2, 128, 3, 5, 62976)))
    for dil, lds in ((1, 123392), (3, 126464), (9, 132608)):
        rows.append((f"k7 64 dil {dil}", dict(Cin=64, Cout=64, ks=7, dil=dil), 7, (FAT, 2, 512, 7, 3, lds)))
    rows.append(("k7 32 dil 9", dict(Cin=32, Cout=32, ks=7, dil=9), 7, (FAT, 1, 512, 7, 3, 121600)))
    for dil, dx, nx, lds in ((1, 7, 3, 156672), (3, 7, 3, 159744), (9, 6, 2, 129024)):
        rows.append((f"fused 96 dil {dil}", dict(Cin=96, Cout=96, ks=7, dil=dil, fused=1), 7, (F96, 6, 512, dx, nx, lds)))
    for dil, lds in ((1, 122880), (3, 125952), (9, 132096)):
        rows.append((f"fused 192 dil {dil}", dict(Cin=192, Cout=192, ks=7, dil=dil, fused=1), 7,
                     (F192, 12, 256, 7, 3, lds)))

    over_80k = set()
    for name, kw, ks, want in rows:
        rc, p = plan(**kw)
        assert rc == 0, (name, lib.zk_last_error())
        assert (p["shape"], p["fm"], p["tile"], p["dx"], p["nx"], p["lds"]) == want, (name, p)
        assert p["lds"] <= 160 * 1024 and p["nx"] == 1 + (p["dx"] + ks) // ks and p["dx"] >= 3, (name, p)
        cot = 16 * p["fm"] * (1 if kw.get("fused") else 2)          # channels per tile
        assert p["nq"] == -(-kw.get("Qn", T) // p["tile"]), (name, p)
        assert p["tiles"] == B * p["nq"] * (kw["Cout"] // cot) * kw.get("nphase", 1), (name, p)
        assert p["wg_per_cu"] == (2 if p["shape"] == PAIR else 1), (name, p)
        if p["shape"] == PAIR and p["lds"] > 80 * 1024:
            over_80k.add(name)
    assert over_80k == {f"1x1+res {c}" for c in (1536, 1024, 768, 512, 384, 256, 128)}

    # what the entries refuse, the query refuses: -1 and a message
    for kw in (dict(Cin=48, Cout=96, ks=7, dil=1), dict(Cin=96, Cout=48, ks=7, dil=1), dict(Cin=96, Cout=96, ks=7, dil=11),
               dict(Cin=96, Cout=96, ks=8, dil=1), dict(Cin=384, Cout=384, ks=7, dil=1, fused=1),
               dict(Cin=96, Cout=96, ks=7, dil=11, fused=1)):
        rc, _ = plan(**kw)
        assert rc == -1 and lib.zk_last_error().startswith(b"zk_dac_conv_plan:"), (kw, rc, lib.zk_last_error())
    assert plan(Cin=96, Cout=96, ks=7, dil=10)[0] == 0               # (ks - 1) * dil = 60 <= 64


def test_gemm_and_gemv_plans_of_product_and_test_shapes(lib):
    """zk_gemm_plan / zk_gemv_plan (the plans zk_gemm_bf16 / zk_gemv_fused launch by) for shapes of the c3 model's
    decode and prefill and for the regime boundaries, each evaluated by hand from gemm_plan / gemv_plan / ws_ncw /
    gf_form of gemm.hip; what the entries refuse, the queries refuse."""
    import ctypes as C
    for fn, n in ((lib.zk_gemm_plan, 5), (lib.zk_gemv_plan, 5)):
        fn.restype = C.c_int
        fn.argtypes = [C.c_int] * n + [C.POINTER(C.c_int32)]
    lib.zk_last_error.restype = C.c_char_p
    RK, WS, PF, TILE = 0, 1, 2, 3
    GF = ("family", "ks", "pf", "nchunks", "mt", "ncw", "u", "ntw", "gx", "gy", "gz", "block", "lds", "pf_cols")
    VF = ("lay", "ksw", "xr", "grid", "block", "ntw", "half", "nw", "ks", "pf")

    def gemm(M, N, K, nsplit=1, mode=0):
        out = (C.c_int32 * 14)()
        return lib.zk_gemm_plan(M, N, K, nsplit, mode, out), dict(zip(GF, out))

    def gemv(M, N, K, mode=0, ln=0):
        out = (C.c_int32 * 10)()
        return lib.zk_gemv_plan(M, N, K, mode, ln, out), dict(zip(VF, out))

    def ws(nch, mt, ncw, gx, gz, mode=0):           # block: ncw compute + loader waves; LDS: 6 slots of mt*16 x 64 bf16
        nld = {(4, 8): 4, (4, 4): 4, (4, 2): 4, (4, 1): 4, (2, 8): 4, (3, 8): 4, (5, 8): 2}[(ncw, mt)]
        return dict(family=WS, pf=4 if mode else 3, nchunks=nch, mt=mt, ncw=ncw, gx=gx, gy=1, gz=gz,
                    block=64 * (ncw + nld), lds=6 * mt * 16 * 64 * 2)

    rows = [
        # decode, B = 64 (128 rows): in_proj split 8, out_proj split 4 (128 workgroups of 4 waves -> 256 of 2),
        # the heads (N = 9234, split 2: 290 -> 232 workgroups of 5 waves), the SwiGLU fc1
        ((128, 3072, 2048, 8), ws(4, 8, 4, 48, 8)),
        ((128, 2048, 2048, 4), ws(8, 8, 2, 64, 4)),
        ((128, 9234, 2048, 2), ws(16, 8, 5, 116, 2)),
        ((128, 16384, 2048, 1, 1), ws(32, 8, 4, 256, 1, mode=1)),
        ((17, 80, 256, 2), ws(2, 2, 4, 2, 2)), ((64, 80, 128, 1), ws(2, 4, 4, 2, 1)),
        # M <= 16: the register-stream GEMV, 2 tiles per workgroup; a slice it has no form for (mode 1, 4 chunks)
        ((16, 80, 256, 1), dict(family=RK, ks=2, pf=2, gx=3, gz=1, block=256, lds=0)),
        ((1, 3072, 2048, 2), dict(family=RK, ks=8, pf=8, gx=96, gz=2, block=256)),
        ((16, 112, 256, 1, 1), ws(4, 1, 4, 2, 1, mode=1)),
        # prefill: 256-row tiles from 256 of them, else k_gemm (two tiles per wave for mode 0 slabs, N >= 512)
        ((16400, 4096, 1024, 1), dict(family=PF, gx=65 * 16, block=512, pf_cols=256)),
        ((9000, 8256, 512, 1, 1), dict(family=PF, gx=36 * 33, pf_cols=256)),
        ((129, 80, 256, 1), dict(family=TILE, u=4, ntw=1, nchunks=4, gx=2, gy=2, gz=1, block=256)),
        ((2048, 384, 2048, 1), dict(family=TILE, u=4, ntw=1, gx=6, gy=16)),
        ((300, 1152, 384, 2), dict(family=TILE, u=1, ntw=2, nchunks=3, gx=9, gy=3, gz=2)),
        ((40, 200, 192, 1), dict(family=TILE, u=1, ntw=1, nchunks=3, gx=4, gy=1)),
        ((8300, 2112, 512, 1), dict(family=PF, gx=33 * 9)),           # (N % 64 == 0 is all the 256-row kernel asks)
        ((8300, 2100, 512, 1), dict(family=TILE, u=4, ntw=2, gx=17, gy=65)),
    ]
    for args, want in rows:
        rc, p = gemm(*args)
        assert rc == 0, (args, lib.zk_last_error())
        assert {k: p[k] for k in want} == want, (args, p)
        if p["family"] != WS:
            assert (p["mt"], p["ncw"]) == (0, 0) and (p["family"] == TILE or p["nchunks"] == 0), (args, p)

    vrows = [
        # B = 1 decode (2 rows): in_proj with the LayerNorm prologue (one tile, 12 k-steps in flight), out_proj
        # (half tiles, 8 waves), fc1 (two tiles), fc2 (K = 8192, half tiles), the heads
        ((2, 3072, 2048, 0, 1), dict(lay=1, ksw=64, xr=2, grid=192, block=256, ntw=1, half=0, nw=4, ks=16, pf=12)),
        ((2, 2048, 2048, 2, 0), dict(lay=0, ksw=64, xr=2, grid=256, block=512, ntw=1, half=1, nw=8, ks=8, pf=4)),
        ((2, 16384, 2048, 1, 1), dict(lay=2, ksw=64, xr=2, grid=512, block=256, ntw=2, half=0, nw=4, ks=16, pf=8)),
        ((2, 2048, 8192, 2, 0), dict(lay=0, ksw=256, xr=2, grid=256, block=512, nw=8, ks=32, pf=8)),
        ((16, 9234, 2048, 0, 1), dict(lay=2, ksw=64, xr=16, grid=289, block=256, ntw=2, pf=8)),
        # the layout edges: 255 / 256 tiles, 511 / 512 tiles; SwiGLU never runs on half tiles
        ((3, 4080, 4096, 0, 0), dict(lay=0, ksw=128, xr=16, grid=510)), ((3, 4096, 4096, 0, 0), dict(lay=1, grid=256)),
        ((3, 8176, 2048, 2, 0), dict(lay=1, grid=511)), ((3, 8192, 2048, 2, 0), dict(lay=2, grid=256)),
        ((3, 8208, 2048, 0, 0), dict(lay=2, grid=257)), ((2, 208, 2048, 1, 0), dict(lay=1, grid=13)),
    ]
    for args, want in vrows:
        rc, p = gemv(*args)
        assert rc == 0, (args, lib.zk_last_error())
        assert {k: p[k] for k in want} == want, (args, p)
        assert p["block"] == 64 * p["nw"] and p["ks"] * p["nw"] == p["ksw"] and p["ntw"] == (2 if p["lay"] == 2 else 1)

    # what the entries refuse, the queries refuse: -1 and a message
    for args in ((0, 10, 64, 1, 0), (4, 10, 100, 1, 0), (4, 10, 256, 3, 0), (4, 24, 256, 1, 1), (4, 32, 256, 2, 1),
                 (4, 32, 256, 1, 2)):
        rc, _ = gemm(*args)
        assert rc == -1 and lib.zk_last_error().startswith(b"zk_gemm_plan:"), (args, rc, lib.zk_last_error())
    for args in ((17, 64, 2048, 0, 0), (0, 64, 2048, 0, 0), (2, 64, 1024, 0, 0), (2, 40, 2048, 1, 0), (2, 64, 2048, 3, 0),
                 (2, 64, 4096, 0, 1)):
        rc, _ = gemv(*args)
        assert rc == -1 and lib.zk_last_error().startswith(b"zk_gemv_plan:"), (args, rc, lib.zk_last_error())


def test_gemm_warm_word_round_trip(lib):
    """The packed warm-up word (warm.h: chunks, NG, compute waves, grid tiles past N) is packed by
    zk_gemm_warm_desc and unpacked by warm_unit's accessors, which zk_gemm_warm_tiles runs on the host: the
    tiles it counts are exactly the grid's 16-column tiles that hold a column < N, for workgroups of 2, 3,
    4 and 5 compute waves and with a non-zero number of grid tiles past N."""
    lib.zk_gemm_warm_tiles.restype = ctypes.c_int
    # (M, N, K, nsplit) -> compute waves per workgroup (the rule of gemm.hip's ws_ncw), grid tiles past N
    cases = [((128, 8512, 2048, 1), 3, 2), ((128, 9234, 2048, 2), 5, 2), ((72, 3000, 512, 1), 2, 0),
             ((128, 3072, 2048, 4), 4, 0), ((24, 1000, 2048, 2), 4, 1), ((128, 2048, 2048, 4), 2, 0)]
    for (M, N, K, nsplit), nw, excess in cases:
        tiles = (N + 15) // 16
        gx = -(-N // (16 * nw))
        assert gx * nw - tiles == excess, (N, nw)          # the case is what its comment says
        for chunks in (1, 2, 4, 40):                       # more chunks than the K slice has: clamped, same tiles
            assert lib.zk_gemm_warm_tiles(M, N, K, nsplit, 0, chunks) == tiles, (M, N, K, nsplit, chunks)
    # (a width or an excess lost in the word would show: N = 8512 unpacked as 4 waves counts 178 x 4 - 2 = 710
    # tiles, without its excess 534, for an image of 532)
    # outside k_gemm_ws's regime (M <= 16; 128 chunks per slice; a prefill M): no warm-up
    for M, N, K, nsplit in ((16, 3072, 2048, 4), (128, 2048, 8192, 1), (300, 3072, 2048, 1)):
        assert lib.zk_gemm_warm_tiles(M, N, K, nsplit, 0, 2) == 0


def test_split_selection_batch_invariant():
    from zonos_amd.engine import _split_for
    for N, K in ((3072, 2048), (2048, 2048), (2048, 8192), (9234, 2048)):
        s = _split_for(N, K, 128)
        assert K % (s * 64) == 0
        assert all(_split_for(N, K, m) == s for m in (2, 8, 64, 128))
        assert ((N + 63) // 64) * s >= 128


def test_attention_split_rule():
    """Flash-decoding key splits: none at B=64 (512 workgroups already), and each split covers
    >= 2048 cached keys (a combine launch costs more than it saves below that)."""
    from zonos_amd.engine import attn_merge_for, attn_splits_for
    # B = 1: 4 splits of 32-key slices at every cache size (round-6 A/B, c2 decode step at
    # 2 / 4 / 8 splits: 0.975-0.978 / 0.959-0.962 / 0.977-0.980 ms, profiles/r6_c2_split_ab.txt)
    assert attn_merge_for(2, 1280) == 4 and attn_merge_for(2, 256) == 4 and attn_merge_for(1 * 2, 3328) == 4
    assert attn_merge_for(4, 1280) == 0 and attn_merge_for(128, 3072) == 0
    assert attn_splits_for(128, 4, 3072) == 1           # c3
    assert attn_splits_for(2, 4, 1280) == 1             # c2: B=1, 10 s
    assert attn_splits_for(2, 4, 3328) == 2             # B=1, 30 s
    for R in (2, 8, 16, 64, 128):
        for smax in (256, 1024, 3072, 8192):
            s = attn_splits_for(R, 4, smax)
            assert 1 <= s <= max(1, smax // 128) and (s == 1 or smax / s >= 1024)


def test_kv_layout_pack_roundtrip():
    """zonos_amd.kvlayout (host view of backbone.hip k_off / v_off): pack/unpack are inverse
    and element positions follow the documented fragment order."""
    import torch
    from zonos_amd.kvlayout import pack_k, pack_v, unpack_k, unpack_v
    R, Hk, S = 2, 3, 64
    k, v = torch.randn(R, Hk, S, 128), torch.randn(R, Hk, S, 128)
    kp, vp = pack_k(k), pack_v(v)
    assert torch.equal(unpack_k(kp, S), k) and torch.equal(unpack_v(vp, S), v)
    for key in (0, 5, 13, 31, 37, 63):
        o = key & 31
        ln = 4 * (o >> 3) + (o & 3)
        h = (o >> 2) & 1
        for c8 in (0, 3, 7, 15):
            off = (key >> 5) * 4096 + ((h * 4 + (c8 >> 2)) * 64 + (c8 & 3) * 16 + ln) * 8
            assert torch.equal(kp[1, 2, off:off + 8], k[1, 2, key, 8 * c8:8 * c8 + 8])
        for ch in (0, 17, 127):
            off = (key >> 5) * 4096 + ((ch >> 4) * 64 + (o >> 3) * 16 + (ch & 15)) * 8 + (o & 7)
            assert vp[1, 2, off] == v[1, 2, key, ch]


def test_struct_layouts_match_header(tmp_path):
    """ctypes mirrors of the by-value/by-pointer structs (ZkCondPlan, sampling params, generation
    state) have the C compiler's size and field offsets."""
    import ctypes as C
    import shutil
    import subprocess

    from zonos_amd import _lib as zl
    from zonos_amd.conditioning import ZkCondPlan, ZkCondSeg
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    hdr = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "zonos_hip.h")
    src = tmp_path / "layout.c"
    src.write_text(f'#include "{hdr}"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(ZkCondSeg), sizeof(ZkCondPlan),'
                   ' offsetof(ZkCondPlan, seg), offsetof(ZkCondSeg, table), offsetof(ZkCondPlan, norm_w),'
                   ' sizeof(zk_sampling_params)); return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(ZkCondSeg), C.sizeof(ZkCondPlan), ZkCondPlan.seg.offset, ZkCondSeg.table.offset,
                   ZkCondPlan.norm_w.offset, C.sizeof(zl.SamplingParams)]


def test_ctypes_struct_layouts_match_the_c_abi(lib):
    """The by-value / by-pointer ABI structs the Python binding builds (SamplingParams, GenState,
    ZkCondSeg, ZkCondPlan, StepLayer, StepDesc, DacDesc) have the C compiler's size and field offsets."""
    import ctypes as C

    from zonos_amd import _lib
    from zonos_amd.conditioning import ZkCondPlan, ZkCondSeg
    lib.zk_abi_size.restype = C.c_long
    lib.zk_abi_size.argtypes = [C.c_int]
    for which, cls in [(0, _lib.SamplingParams), (1, _lib.GenState), (4, ZkCondSeg), (5, ZkCondPlan)]:
        assert lib.zk_abi_size(which) == C.sizeof(cls), (cls.__name__, lib.zk_abi_size(which), C.sizeof(cls))
    assert lib.zk_abi_size(12) == _lib.GenState.seed.offset
    assert lib.zk_abi_size(22) == _lib.GenState.noise_offset.offset
    assert lib.zk_abi_size(6) == C.sizeof(_lib.StepLayer) and lib.zk_abi_size(7) == C.sizeof(_lib.StepDesc)
    assert lib.zk_abi_size(13) == _lib.StepDesc.eps.offset
    assert lib.zk_abi_size(14) == _lib.StepDesc.st.offset and lib.zk_abi_size(15) == _lib.StepDesc.sp.offset
    assert lib.zk_abi_size(8) == C.sizeof(_lib.DacDesc) and lib.zk_abi_size(17) == C.sizeof(_lib.DacBlock)
    assert lib.zk_abi_size(16) == _lib.DacDesc.blocks.offset
    assert lib.zk_abi_size(18) == C.sizeof(_lib.HybridLayer) and lib.zk_abi_size(19) == C.sizeof(_lib.HybridDesc)
    assert lib.zk_abi_size(20) == _lib.HybridDesc.st.offset and lib.zk_abi_size(21) == _lib.HybridDesc.eps.offset


