"""csrc/conv_tiles.h (which conv tile may run which convolution -- the class table of every family, the launch-level rule at every clause with its smallest refusing
neighbour -- and the tile counts of a launch), under the host sanitizers: tests/conv_tiles_host.hip is a program of its own, built with -fsanitize=address,undefined
on the host side and run directly -- never through Python, never on a GPU (it makes no HIP call).  Also, on the source text: the rule, the tile counts and the LDS
size of an implicit-GEMM tile each have one home, and no source tells a family by an integer any more."""
import os
import re
import shutil
import subprocess

import pytest

from head_detector_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "head_detector_amd", "csrc")


@pytest.mark.parametrize("define", [None, "-DVGH_EXPERIMENTS"])
def test_tile_rule_and_tile_counts_under_sanitizers(tmp_path, define):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "conv_tiles_host")
    cc = [hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Wno-unused-result", "-Wno-unused-value", *([define] if define else []), "-Xarch_host", "-fsanitize=address,undefined",
          "-Xarch_host", "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "conv_tiles_host.hip"), "-o", exe]
    r = subprocess.run(cc, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    nm = subprocess.run(["nm", exe], capture_output=True, text=True, check=True).stdout
    assert "__asan_init" in nm and "__ubsan_handle" in nm  # the host code really is instrumented
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "conv_tiles host checks passed" in r.stdout, r.stdout + r.stderr
    assert f"{64 if define else 62} launch cases" in r.stdout, r.stdout  # the d tiles' two cases exist in the experiments build only


def test_tile_rule_has_one_home():
    claimed = {f for c in build.COMPANIONS for f in c.sources + c.headers}
    text = {f: open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith((".hip", ".h", ".inc")) and f not in claimed}  # every source of libvgh.so
    assert {"conv_tiles.h", "conv_args.h", "conv_igemm.hip", "conv_split.hip", "conv_pp.hip", "ds_b2b.hip"} <= set(text) and set(build.SOURCES + build.EXPERIMENT_SOURCES) <= set(text)
    host = open(os.path.join(ROOT, "tests", "conv_tiles_host.hip")).read()
    assert re.findall(r'#include "([^"]+)"', host) == ["../head_detector_amd/csrc/conv_tiles.h"] and "hip" not in " ".join(re.findall(r"#include <([^>]+)>", host))

    def homes(pattern):
        return sorted(f for f, s in text.items() for _ in re.findall(pattern, s))

    # plain data and host logic: no HIP include, directly or through another header
    assert re.findall(r"#include\s+(\S+)", text["conv_args.h"]) == ["<stdint.h>"]
    assert re.findall(r"#include\s+(\S+)", text["conv_tiles.h"]) == ["<stdint.h>", '"../../include/vgh.h"', '"conv_args.h"']
    assert re.findall(r"#include\s+(\S+)", open(os.path.join(ROOT, "include", "vgh.h")).read()) == ["<stdint.h>"]
    assert homes(r"\bstruct ConvArgs \{") == ["conv_args.h"] and '#include "conv_tiles.h"' in text["vgh_internal.h"]
    # a family is a TileFamily, never an integer; one launcher type
    for gone in (r"patch ==", r"patch !=", r"\blaunch_patch\b", r"\bkPPBC\b", r"\bpp16_ok\b", r"\bigemm_lds\b", r"static bool resolved"):
        assert homes(gone) == [], (gone, homes(gone))
    assert homes(r"\bTileFamily family;") == ["conv_igemm.hip", "conv_split.hip"] and homes(r"VGH_TILE_LAUNCHER\(\(\*launch\)\);") == ["conv_igemm.hip", "conv_split.hip"]
    assert homes(r"#define VGH_TILE_LAUNCHER") == ["vgh_internal.h"]
    # the rule, its predicates, the tile counts and the LDS size: defined in conv_tiles.h alone
    for defined in (r"\bbool tile_admits\(", r"\bbool tile_class_admits\(", r"\bbool tile_grid\(", r"\bint vgh_conv_pp_fits\(", r"\bint vgh_conv_ds_ok\(", r"\bint vgh_conv_w_ok\(",
                    r"\bint vgh_conv_ds_b2b_ok\(", r"\bint vgh_conv_b2b_ok\(", r"constexpr int lds_bytes\("):
        assert homes(defined) == ["conv_tiles.h"], (defined, homes(defined))
    assert homes(r"\(total \+ 7\) / 8") == ["conv_tiles.h", "ds_b2b.hip"]  # ds_b2b.hip: persistent_grid rounds its chunk to whole pixel tiles
    assert homes(r"cout_pad / (e\.)?BC\b") == ["conv_tiles.h"] and homes(r"total < \(1ll << 30\)|total >= \(1ll << 30\)") == ["conv_tiles.h", "ds_b2b.hip"]  # ds_b2b.hip: the t / u pair
    assert text["conv_igemm.hip"].count("tile_grid(") == 2 and text["conv_split.hip"].count("tile_grid(") == 1  # vgh_launch_conv and the b2b tile; vgh_launch_conv_split
    # the launchers of conv_pp.hip and ds_b2b.hip still refuse what their own predicate refuses
    assert "VGH_REQUIRE(vgh_conv_pp_fits(a)" in text["conv_pp.hip"]
    for pred in ("vgh_conv_ds_ok", "vgh_conv_w_ok", "vgh_conv_ds_b2b_ok"):
        assert f"VGH_REQUIRE({pred}(a)" in text["ds_b2b.hip"], pred
