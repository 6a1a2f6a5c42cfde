"""The register and LDS budget that lets a K(X*,X) producer workgroup sit beside two predict-GEMM workgroups on a CU
(option streams=3), read from the shipped code object's notes -- no GPU needed.  Per SIMD: two GEMM waves and one producer
wave, 2 x 176 + 152 = 504 <= 512 VGPRs (allocation granule 8); per CU: 2 x 73 728 B of LDS <= 160 KB, the producer none."""
import os
import re
import shutil
import subprocess

import pytest

from spearmint_amd import engine

LLVM = "/opt/rocm/lib/llvm/bin"
GEMM_VGPRS, CORUN_VGPRS, GEMM_LDS = 176, 152, 73728


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{kernel name: {note field: int}} over every gfx950 code object in libspx.so"""
    if not os.path.exists(os.path.join(LLVM, "clang-offload-bundler")):
        pytest.skip("no ROCm llvm tools on this box")
    tmp = tmp_path_factory.mktemp("notes")
    so = str(tmp / "libspx.so")
    shutil.copy(engine.default_lib_path(), so)
    subprocess.check_call([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], stdout=subprocess.DEVNULL)
    objs = [f for f in os.listdir(str(tmp)) if "amdgcn" in f]
    assert objs, "no gfx950 code objects found in libspx.so"
    out = {}
    for f in objs:
        notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", str(tmp / f)]).decode()
        for blk in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
            d = dict(re.findall(r"\.(\w+):\s+(\S+)", ".agpr_count:" + blk.split("\namdhsa.")[0]))
            out[d["name"]] = {k: int(v) for k, v in d.items() if re.fullmatch(r"\d+", v)}
    assert len(out) > 40, sorted(out)
    return out


def test_production_gemm_kernels_leave_room_for_a_producer_wave(kernels):
    gemm = {k: v for k, v in kernels.items() if "k_predict_gemm_tri" in k or "k_predict_gemm_tail" in k}
    assert len(gemm) == 4, sorted(gemm)            # tri, tail<1>, tail<2>, tail<3>
    for name, n in gemm.items():
        assert n["vgpr_count"] <= GEMM_VGPRS, (name, n["vgpr_count"])
        assert n["agpr_count"] == 0, name          # AGPR accumulators halve the fp64 MFMA rate
        assert n["private_segment_fixed_size"] == 0 and n.get("vgpr_spill_count", 0) == 0, name
        assert n["group_segment_fixed_size"] == 0, name     # all of its LDS is the launcher's dynamic allocation ...
    lib = engine.load_library()
    h = engine.ctypes.c_void_p()
    assert lib.spx_create(0, engine.ctypes.byref(h)) == 0   # (no device is touched before the first call that needs one)
    try:
        v = engine.ctypes.c_int64(0)
        assert lib.spx_get_stat(h, b"gemm_lds_bytes", engine.ctypes.byref(v)) == 0
        assert v.value == GEMM_LDS                           # ... which is this
    finally:
        lib.spx_destroy(h)
    assert 2 * GEMM_LDS <= 160 * 1024


def test_corun_producer_fits_beside_two_gemm_workgroups(kernels):
    corun = {k: v for k, v in kernels.items() if "k_cov_corun" in k}
    assert len(corun) == 9, sorted(corun)          # QC 1 / 2 / 4 x three correlation functions
    for name, n in corun.items():
        assert n["vgpr_count"] <= CORUN_VGPRS, (name, n["vgpr_count"])
        assert n["agpr_count"] == 0, name
        assert n["group_segment_fixed_size"] == 0, name
        assert n["private_segment_fixed_size"] == 0 and n.get("vgpr_spill_count", 0) == 0, name
    # VGPRs are allocated in granules of 8 per wave
    def gran(x):
        return -(-x // 8) * 8
    worst_gemm = max(v["vgpr_count"] for k, v in kernels.items() if "k_predict_gemm_t" in k)
    worst_corun = max(v["vgpr_count"] for v in corun.values())
    assert 2 * gran(worst_gemm) + gran(worst_corun) <= 512
