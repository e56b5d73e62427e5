"""The deferrable-op marks and the pending state of csrc/net_plan.h (vgh_net_set_defer / vgh_net_run_deferred) under the host sanitizers, on the L and M programs:
tests/deferred_plan_host.hip is a program of its own, built with -fsanitize=address,undefined on the host side and run directly -- never through Python, never on
a GPU.  The plan has to find, from the descriptors alone, exactly the nine final 1x1 convs of the FLAME towers (three per level); the names are used here only to say
which ops those are."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import pytest

from head_detector_amd import _lib, arch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dump(path, variant, image_size=64):
    P = arch.build_program(variant, arch.random_state_dict(variant, 1), image_size, "bf16")
    w, b = P.arrays()
    bufs = (_lib.BufDesc * len(P.bufs))(*[_lib.BufDesc(bf["h"], bf["w"], bf["pitch"], bf["is_f32"], float(bf.get("scale", 0.0))) for bf in P.bufs])
    fields = [f for f, _ in _lib.OpDesc._fields_]
    ops = (_lib.OpDesc * len(P.ops))(*[_lib.OpDesc(**{f: (op.get(f, 0) if f != "in_buf" else max(op[f], 0)) for f in fields}) for op in P.ops])
    expected = [i for i, op in enumerate(P.ops) if re.fullmatch(r"heads\.head\d\.flame_(shape|expression|transform)_pred\.(\d+)", op["name"]) and op["ksize"] == 1]
    assert len(expected) == 9 and all(P.bufs[P.ops[i]["out_buf"]]["is_f32"] == arch.FMT_F32 for i in expected)
    with open(path, "wb") as f:
        f.write(struct.pack("<8q", image_size, len(P.bufs), len(P.ops), w.size, b.size, C.sizeof(_lib.BufDesc), C.sizeof(_lib.OpDesc), len(expected)))
        f.write(struct.pack(f"<{len(expected)}i", *expected))
        f.write(bytes(bufs))
        f.write(bytes(ops))
    return expected


def test_deferrable_marks_and_pending_state_under_sanitizers(tmp_path):
    files = []
    for variant in ("vgg_heads_l", "vgg_heads_m") if "vgg_heads_m" in arch.VARIANTS else sorted(arch.VARIANTS):
        files.append(str(tmp_path / f"{variant}.prog"))
        _dump(files[-1], variant)
    assert len(files) >= 2
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "deferred_plan_host")
    cc = [hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Wno-unused-result", "-Wno-unused-value", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
          "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "deferred_plan_host.hip"), "-o", exe]
    r = subprocess.run(cc, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    nm = subprocess.run(["nm", exe], capture_output=True, text=True, check=True).stdout
    assert "__asan_init" in nm and "__ubsan_handle" in nm  # the host code really is instrumented
    r = subprocess.run([exe, *files], capture_output=True, text=True, timeout=300)  # (LeakSanitizer runs at exit: a leak is a non-zero status)
    assert r.returncode == 0 and "deferred plan host checks passed" in r.stdout, r.stdout + r.stderr


def test_the_switch_is_off_by_default_and_the_executor_skips_in_one_place():
    net = open(os.path.join(ROOT, "head_detector_amd", "csrc", "net.hip")).read()
    plan = open(os.path.join(ROOT, "head_detector_amd", "csrc", "net_plan.h")).read()
    assert "bool on = false;" in plan and net.count("op.deferrable) return VGH_OK;") == 1
    # no op names in the rule: the mark comes from the descriptors
    rule = plan[plan.index("inline bool net_op_deferrable("):plan.index("struct DeferState")]
    assert "name" not in rule and "flame" not in rule.lower().replace("vgh_pred_flame_off", "")
