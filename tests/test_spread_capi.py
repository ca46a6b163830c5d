"""srsgpu_tdec_latency_form (host code, no GPU): which block sizes a small job decodes on the
latency kernel k_win_spread — every size a windowed decoder takes — and the kernel's scratch budget
(a cross-compile of the 16-sub-block decoder part with the compiler's resource-usage remarks)."""
import ctypes
import os
import re
import subprocess

import pytest

from srsgpu_testlib import AUTO, AVX_WINDOW, SSE, SSE_WINDOW, cb_sizes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "empower-srslte_amd", "lib", "libsrsgpu_phy.so")
HIPCC = "/opt/rocm/bin/hipcc"
AUTO8 = 16  # SRSGPU_TDEC_AUTO_8BIT


def test_latency_form_is_exported_and_mirrored():
    lib = ctypes.CDLL(LIB)
    assert hasattr(lib, "srsgpu_tdec_latency_form")
    import srsgpu_phy as s
    assert "srsgpu_tdec_latency_form" in s.EXPORTED
    assert s.latency_form(AUTO, 6144) == 1


def test_every_windowed_size_takes_the_latency_form():
    import srsgpu_phy as s
    sizes = cb_sizes()
    assert len(sizes) == 188
    win = [K for K in sizes if s.autoimp_get_subblocks(K) != 0]
    assert len(win) == 142
    for K in sizes:
        assert s.latency_form(AUTO, K) == (1 if K in win else 0), K
    assert s.latency_form(AUTO, 5824) == 1  # the headline block size: L = 364, a partial last chunk
    # the 8-bit AUTO choice: windowed exactly where it picks sub-blocks
    lib = ctypes.CDLL(LIB)
    lib.srslte_tdec_autoimp_get_subblocks_8bit.restype = ctypes.c_uint32
    lib.srslte_tdec_autoimp_get_subblocks_8bit.argtypes = [ctypes.c_uint32]
    for K in sizes:
        assert s.latency_form(AUTO8, K) == (1 if lib.srslte_tdec_autoimp_get_subblocks_8bit(K) != 0 else 0), K


def test_latency_form_refusals_and_manual_types():
    import srsgpu_phy as s
    assert s.latency_form(AUTO, 41) == -1          # no LTE block size
    assert s.latency_form(99, 6144) == -1          # no decoder type
    assert s.latency_form(-1, 6144) == -1
    assert s.latency_form(SSE, 6144) == 0          # sequential decoder: throughput kernels
    assert s.latency_form(AVX_WINDOW, 656) == 1    # L = 41, the smallest a window decoder takes
    assert s.latency_form(AVX_WINDOW, 640) == -1   # L = 40: refused by the engine
    assert s.latency_form(SSE_WINDOW, 408) == 1
    assert s.latency_form(AVX_WINDOW, 408) == -1   # 408 is no multiple of 16


def _usage(src):
    """{kernel (mangled): {"VGPRs": n, "ScratchSize": n, ...}} from -Rpass-analysis=kernel-resource-usage"""
    out = subprocess.run([HIPCC, "-O3", "-fPIC", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950",
                          "-I" + os.path.join(REPO, "include"), "-I" + os.path.join(REPO, "empower-srslte_amd", "csrc"),
                          "-c", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    res, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[bytes/lane\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return res


# ScratchSize of every k_win_spread instantiation of tdec_part_w16.hip at commit ec4ec37 (before the
# partial chunk: six instantiations, 207-224 VGPRs), by the command of _usage
PARENT_SPREAD_SCRATCH = 0


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_spread_kernel_keeps_its_metrics_in_registers():
    """the partial chunk's selects and guards must not push k_win_spread's 16 beta states per task
    out of the register file"""
    u = _usage(os.path.join(REPO, "empower-srslte_amd", "csrc", "tdec_part_w16.hip"))
    names = {k: v for k, v in u.items() if "k_win_spread" in k}
    assert len(names) == 12, list(u)  # three modes, with and without decisions, whole chunks / a partial one
    for k, v in names.items():
        assert v.get("ScratchSize", 0) <= PARENT_SPREAD_SCRATCH, (k, v)
