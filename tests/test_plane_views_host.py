"""Host part of csrc/plane_views.h (pair_of, plane_range, in_place, chan_of, the checks of a plane and the overlap rule with every message in both label
styles) under the host sanitizers: tests/plane_views_host.hip is a program of its own, built with -fsanitize=address,undefined on the host side and run
directly -- never through Python, never on a GPU (it makes no HIP call)."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plane_checks_and_pair_rule_under_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "plane_views_host")
    cc = [hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Wno-unused-result", "-Wno-unused-value", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
          "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "plane_views_host.hip"), "-o", exe]
    r = subprocess.run(cc, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    nm = subprocess.run(["nm", exe], capture_output=True, text=True, check=True).stdout
    assert "__asan_init" in nm and "__ubsan_handle" in nm  # the host code really is instrumented
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "plane_views host checks passed" in r.stdout, r.stdout + r.stderr


def test_the_program_includes_the_header_alone():
    host = open(os.path.join(ROOT, "tests", "plane_views_host.hip")).read()
    assert re.findall(r'#include "([^"]+)"', host) == ["../head_detector_amd/csrc/plane_views.h"] and "hip" not in " ".join(re.findall(r"#include <([^>]+)>", host))
