"""csrc/flame_plan.h (which kernels a FLAME decode runs: the table at every threshold and its neighbours, expected values printed by the if-chain the function
replaced) and csrc/per_device.h (the once-per-device routine with a counting callable, the slot function), under the host sanitizers:
tests/flame_plan_host.hip is a program of its own, built with -fsanitize=address,undefined on the host side and run directly -- never through Python, never
on a GPU (it makes no HIP call).  Also: the per-device launch state and the decode's thresholds are defined once.  What a second GPU would show -- an opt-in per
device -- is tested here on the host only: the GPU suite cannot assume one."""
import os
import re
import shutil
import subprocess

import pytest

from head_detector_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "head_detector_amd", "csrc")


@pytest.mark.parametrize("define", [None, "-DVGH_EXPERIMENTS"])
def test_plan_table_and_once_per_device_under_sanitizers(tmp_path, define):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "flame_plan_host")
    cc = [hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Wno-unused-result", "-Wno-unused-value", *([define] if define else []), "-Xarch_host", "-fsanitize=address,undefined",
          "-Xarch_host", "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "flame_plan_host.hip"), "-o", exe]
    r = subprocess.run(cc, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    nm = subprocess.run(["nm", exe], capture_output=True, text=True, check=True).stdout
    assert "__asan_init" in nm and "__ubsan_handle" in nm  # the host code really is instrumented
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "flame_plan and per_device host checks passed" in r.stdout, r.stdout + r.stderr
    # the head counts the GPU bit-identity tests (test_gpu_parity.py, test_gpu_flame_cases.py) must run in automatic mode to reach every plan value
    first = [(kind, int(m), k) for kind, m, k in re.findall(r"first (batch|capacity) of +(\d+): (\w+)", r.stdout)]
    assert first == [("batch", 1, "C3Fused1"), ("batch", 2, "C3Fused2"), ("batch", 3, "C3Fused4"), ("batch", 5, "C3Fused8"), ("batch", 9, "C3Waves5"), ("batch", 33, "C3Waves1"),
                     ("batch", 97, "C3V128"), ("batch", 193, "C3V160"), ("batch", 257, "C3V128H64"), ("batch", 2049, "Lds128"), ("capacity", 1, "C3Waves1"), ("capacity", 129, "C3V128"),
                     ("capacity", 16385, "Valu8")], r.stdout


def test_launch_state_and_thresholds_are_defined_once():
    claimed = {f for c in build.COMPANIONS for f in c.sources + c.headers}
    text = {f: open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith((".hip", ".h", ".inc")) and f not in claimed}  # every source of libvgh.so
    assert {"per_device.h", "flame_plan.h", "flame.hip", "streams.hip", "stem_pool.hip", "stem_ds.hip"} <= set(text) and set(build.SOURCES + build.EXPERIMENT_SOURCES) <= set(text)

    def homes(pattern):
        return sorted(f for f, s in text.items() for _ in re.findall(pattern, s))

    for gone in (r"\bkMaxDev\b", r"cur_dev\(", r"current_device\(", r"attr_done", r"static bool attr"):
        assert homes(gone) == [], (gone, homes(gone))
    assert homes(r"kMaxDevices =") == ["per_device.h"] and homes(r"hipGetDevice\(&\w+\) != hipSuccess") == []
    # the dynamic-LDS opt-in: per_device.h, and stem_pool.hip's three per-call opt-ins (its LDS size varies with the map)
    assert homes(r"hipFuncAttributeMaxDynamicSharedMemorySize") == ["per_device.h"] * 2 + ["stem_pool.hip"] * 3
    assert homes(r"hipOccupancyMaxActiveBlocksPerMultiprocessor") == ["per_device.h"]
    for f in ("conv_cfg_list.h", "ds_b2b.hip", "conv_pp.hip", "conv_split.hip", "flame.hip", "streams.hip"):
        assert '#include "per_device.h"' in text[f], f
    # the decode's choice: thresholds and conditions in flame_plan.h only, which includes nothing (no HIP)
    for threshold in ("kLdsMinHeads", "kC3MaxHeads", "kLdsMidHeads"):
        assert set(homes(threshold)) == {"flame_plan.h"}, (threshold, homes(threshold))
    assert "#include" not in text["flame_plan.h"] and text["flame.hip"].count("flame_plan(") == 1
    for launch in (r"launch_c3<\d", r"launch_mfma_lds<\d", r"launch_mfma<\d", r"launch_vertex_cfg<\d"):  # flame.hip launches by the plan's list alone
        assert set(homes(launch)) == {"flame_plan.h"}, (launch, homes(launch))
    # one persistent grid width for the t / u, r and w tiles
    assert text["ds_b2b.hip"].count("persistent_grid(a, total, ") == 3 and text["ds_b2b.hip"].count("DT_FULL_WIDTH ?") == 1
