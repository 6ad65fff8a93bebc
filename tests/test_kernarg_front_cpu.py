"""CPU: the front of the decode-step kernels in the device assembly, built with the library's own flags
(zonos_amd.build.FLAGS, not restated here; DESIGN §6 "Kernel-argument preload").

For every kernel family a c3 / c2 / c5 decode step launches, two things are read out of the `.s`
(tools/resource_report.py kernel_fronts): the number of argument dwords delivered in SGPRs at wave start, and
the scalar loads from the kernarg pointer between the kernel's real entry (behind the compatibility prologue)
and its first vector-memory load, with whether an s_waitcnt waits for them there.

CLEAN families have what the preload is for: a nonzero preload that covers everything the front uses, so no
argument load at all in front of the first data load (for k_gemm_ws and the non-WARM k_resid_ln_d2k512 that is
what their argument order establishes: moving `skip` back behind the 14th dword fails here). The WARM
k_resid_ln_d2k512 may issue, and must not wait for, the loads of its epilogue-only arguments.

The OTHER families were not re-ordered. Their fronts still wait for argument loads; the exact loads are pinned
here as recorded values, so that they can neither grow unseen nor be mistaken for done:
  k_embed_ln 13 dw (the 14th would split a pointer), k_resid_ln / k_resid_ln_var 13 dw: `skip` at 0x50;
  k_attn_decode* 14 dw: out / skip / part (0x48-0x5f) and for the FP8 form 0x40-0x67 lie behind the preload;
  k_gemv_f 14 dw: the LayerNorm / merge / RoPE descriptors behind 0x48; k_gemv_w8 (the same body behind
  another entry kernel) 14 dw: only the merge descriptor (0x58-0x63) is waited for;
  k_mamba_step_g 14 dw: 0x38-0x4f and the step word's pointer at 0x70;
  k_sample_heads 3 dw and k_eos_step 0: zk_gen_state is passed by value, which ends the preload where the
  struct begins (k_eos_step: first argument), and the whole struct is loaded and waited for."""
import importlib.util
import os
import re
import shutil
from concurrent.futures import ThreadPoolExecutor

import pytest

from zonos_amd import build as zb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(not (os.path.exists(zb.HIPCC) or shutil.which(zb.HIPCC)), reason="needs hipcc")

# family -> preload dwords; no argument load before the first vector-memory load
CLEAN = {
    ("gemm.hip", "k_gemm_ws"): 14,
    ("gemm.hip", "k_gemv_rk"): 14,
    ("backbone.hip", "k_attn_combine"): 10,
    ("mamba.hip", "k_gated_norm"): 12,
}
# k_resid_ln_d2k512<NS, WARM>: 14 dwords; WARM may issue (not wait for) x_out / xn_out (0x38) and wW (0x48)
D2K512_WARM_ISSUED = {(0x38, 16), (0x48, 8)}
# family -> (preload dwords, every set of waited-for front loads (offset, bytes) an instantiation has)
OTHER = {
    ("backbone.hip", "k_embed_ln"): (13, [{(0x70, 16), (0x50, 8), (0x40, 8), (0x38, 8)}, {(0x70, 16), (0x38, 32)}]),
    ("backbone.hip", "k_resid_ln"): (13, [{(0x50, 8)}]),
    ("backbone.hip", "k_resid_ln_var"): (13, [{(0x50, 8)}]),
    ("backbone.hip", "k_attn_decode"): (14, [{(0x48, 16)}, {(0x48, 16), (0x58, 8)}]),
    ("backbone.hip", "k_attn_decode_qs"): (14, [{(0x40, 8), (0x48, 4)}]),
    ("backbone.hip", "k_attn_decode_f8"): (14, [{(0x58, 16), (0x40, 16)}]),
    ("gemm.hip", "k_gemv_f"): (14, [set(), {(0x48, 8)}, {(0x68, 32), (0x88, 16)}, {(0x58, 8), (0x60, 4)}]),
    ("gemm.hip", "k_gemv_w8"): (14, [set(), {(0x58, 8), (0x60, 4)}]),
    ("mamba.hip", "k_mamba_step_g"): (14, [{(0x38, 8)}, {(0x38, 16), (0x48, 8), (0x70, 8)}, {(0x38, 8), (0x40, 16), (0x70, 8)}]),
    ("sampler.hip", "k_sample_heads"): (3, [{(0x60, 16), (0xb8, 8), (0x10, 16), (0x38, 32)},
                                            {(0x60, 16), (0xb0, 16), (0x10, 16), (0x38, 32)}]),
    ("sampler.hip", "k_eos_step"): (0, [{(0x80, 8), (0x00, 64), (0x40, 32)}]),
}


@pytest.fixture(scope="module")
def fronts():
    spec = importlib.util.spec_from_file_location("resource_report", os.path.join(ROOT, "tools", "resource_report.py"))
    rr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rr)
    srcs = sorted({s for s, _ in list(CLEAN) + list(OTHER)} | {"backbone.hip"})
    with ThreadPoolExecutor(max_workers=len(srcs)) as ex:
        return dict(zip(srcs, ex.map(lambda s: rr.kernel_fronts(rr.device_asm(s)), srcs)))


def _family(fronts, src, base):
    # Itanium mangling: <length><name>, then template arguments (I) or the end of the nested name (E)
    hits = {k: v for k, v in fronts[src].items() if re.search(r"%d%s[IE]" % (len(base), base), k)}
    assert hits, f"{src}: no kernel {base} in the device assembly"
    return hits


@pytest.mark.parametrize("src,base", sorted(CLEAN))
def test_front_needs_no_argument_load(fronts, src, base):
    for k, v in _family(fronts, src, base).items():
        assert v["preload"] == CLEAN[(src, base)], f"{k}: preloads {v['preload']} argument dwords"
        assert v["front"] == [], f"{k}: argument loads before the first vector-memory load: {v['front']}"


def test_resid_ln_d2k512_front(fronts):
    hits = _family(fronts, "backbone.hip", "k_resid_ln_d2k512")
    assert len(hits) == 6
    for k, v in hits.items():
        warm = "Lb1E" in k
        assert v["preload"] == 14, f"{k}: preloads {v['preload']} argument dwords"
        assert v["waited"] == [], f"{k}: waits for argument loads before its row loads: {v['waited']}"
        assert set(v["front"]) <= (D2K512_WARM_ISSUED if warm else set()), f"{k}: front loads {v['front']}"


@pytest.mark.parametrize("src,base", sorted(OTHER))
def test_front_as_recorded(fronts, src, base):
    preload, recorded = OTHER[(src, base)]
    seen = []
    for k, v in _family(fronts, src, base).items():
        assert v["preload"] == preload, f"{k}: preloads {v['preload']} argument dwords, recorded {preload}"
        assert set(v["waited"]) in recorded, f"{k}: waits for {v['waited']} before its first vector-memory load"
        seen.append(set(v["waited"]))
    assert all(r in seen for r in recorded), f"{base}: a recorded front no longer occurs: update the record"
