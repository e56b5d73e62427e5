"""csrc/net_plan.h (what vgh_net_create decides about a program before its first HIP call: every refusal, the arena and weight-blob offsets, the stem pair and the
back-to-back marks, the cross-lane events and the wait cycle, the lane split, the descriptor -> ConvArgs filler), under the host sanitizers:
tests/net_plan_host.hip is a program of its own, built with -fsanitize=address,undefined on the host side and run directly -- never through Python, never
on a GPU (it makes no HIP call).  Also, on the source text: the plan includes no HIP, and what net.hip wrote two or three times has one home."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "head_detector_amd", "csrc")


@pytest.mark.parametrize("define", [None, "-DVGH_EXPERIMENTS"])
def test_program_plan_under_sanitizers(tmp_path, define):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "net_plan_host")
    cc = [hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Wno-unused-result", "-Wno-unused-value", *([define] if define else []), "-Xarch_host", "-fsanitize=address,undefined",
          "-Xarch_host", "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "net_plan_host.hip"), "-o", exe]
    r = subprocess.run(cc, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    nm = subprocess.run(["nm", exe], capture_output=True, text=True, check=True).stdout
    assert "__asan_init" in nm and "__ubsan_handle" in nm  # the host code really is instrumented
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)  # (LeakSanitizer runs at exit: a leak is a non-zero status)
    assert r.returncode == 0 and "net_plan host checks passed" in r.stdout, r.stdout + r.stderr


def test_the_plan_is_hip_free_and_the_executor_says_things_once():
    text = {f: open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith((".hip", ".h", ".inc"))}
    plan, net = text["net_plan.h"], text["net.hip"]
    host = open(os.path.join(ROOT, "tests", "net_plan_host.hip")).read()
    assert re.findall(r'#include "([^"]+)"', host) == ["../head_detector_amd/csrc/net_plan.h"] and "hip" not in " ".join(re.findall(r"#include <([^>]+)>", host))
    # no HIP in the plan, directly or through what it includes (conv_tiles.h and conv_args.h: tests/test_conv_tiles_host.py)
    assert "#include <hip" not in plan and not re.search(r"\bhip[A-Z]\w*\(", plan)
    assert re.findall(r'#include "([^"]+)"', plan) == ["../../include/vgh.h", "conv_tiles.h"]
    assert '#include "net_plan.h"' in net

    def homes(pattern):
        return sorted(f for f, s in text.items() for _ in re.findall(pattern, s))

    assert homes(r"Ho = \(") == ["net_plan.h"]  # one descriptor -> ConvArgs filler, used by the executor and by vgh_conv2d
    assert net.count("conv_args_fill(") == 2 and homes(r"void conv_args_fill\(") == ["net_plan.h"]
    assert homes(r"B / L \+") == ["net_plan.h"] and net.count("rows_of_lane(") == 2  # the lane split: net_forward_split and vgh_net_profile
    assert net.count("is not a canvas") == 1 and net.count("require_canvas(") == 4  # one check, three callers
    assert homes(r"stem3_ok == 1") == ["net.hip"] and net.count("stem_in_pair_launch(n)") == 2  # net_run_op and vgh_net_stem_fused
    assert homes(r"bool sole_link\(") == ["net_plan.h"] and plan.count("sole_link(ops") == 2 and "in_buf == a.out_buf ||" not in net  # the "nobody else touches it" scan
    assert homes(r"\bg_zeros\[16\]") == [] and "return vgh_launch_conv(a, d.force_cfg, st);" not in net
    # vgh_net_create: the plan before the first HIP call, then a guard instead of hand-written destroys
    create = net[net.index("int vgh_net_create("):net.index("void vgh_net_destroy(")]
    assert "vgh_net_destroy(n);" not in create and "std::unique_ptr<vgh_net" in create and "guard.release()" in create
    first_hip = re.search(r"\bhip[A-Z]\w*\(", create)
    assert first_hip and first_hip.group(0) == "hipSetDevice(" and create.index("net_plan(") < first_hip.start()
