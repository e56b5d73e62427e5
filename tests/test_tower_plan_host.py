"""The tower-deferrable marks of csrc/tower_plan.h and the chain traits of csrc/conv_tiles.h under the host sanitizers, on the L and M programs:
tests/tower_plan_host.hip is a program of its own, built with -fsanitize=address,undefined on the host side and run directly -- never through Python, never on a GPU.
The plan has to find, from the descriptors alone, exactly the 3x3 convs of the FLAME towers in front of the nine deferred 1x1 convs: 21 on L (three layers per level:
the fused layer 0, then shape / expression / grouped transform twice) and 12 on M (two layers per level); the names are used here only to say which ops those are."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

from head_detector_amd import _lib, arch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = {"vgg_heads_l": (21, 3), "vgg_heads_m": (12, 2)}  # tower ops, layers


def _dump(path, variant, image_size=64):
    P = arch.build_program(variant, arch.random_state_dict(variant, 1), image_size, "bf16")
    w, b = P.arrays()
    bufs = (_lib.BufDesc * len(P.bufs))(*[_lib.BufDesc(bf["h"], bf["w"], bf["pitch"], bf["is_f32"], float(bf.get("scale", 0.0))) for bf in P.bufs])
    fields = [f for f, _ in _lib.OpDesc._fields_]
    ops = (_lib.OpDesc * len(P.ops))(*[_lib.OpDesc(**{f: (op.get(f, 0) if f != "in_buf" else max(op[f], 0)) for f in fields}) for op in P.ops])
    flame = [i for i, op in enumerate(P.ops) if re.fullmatch(r"heads\.head\d\.flame_(\*|shape|expression|transform)_pred\.(\d+)", op["name"])]
    towers = [i for i in flame if P.ops[i]["ksize"] == 3]
    preds = [i for i in flame if P.ops[i]["ksize"] == 1]
    n, depth = EXPECTED[variant]
    assert len(towers) == n and len(preds) == 9
    with open(path, "wb") as f:
        f.write(struct.pack("<10q", image_size, len(P.bufs), len(P.ops), w.size, b.size, C.sizeof(_lib.BufDesc), C.sizeof(_lib.OpDesc), len(towers), len(preds), depth))
        f.write(struct.pack(f"<{len(towers) + len(preds)}i", *towers, *preds))
        f.write(bytes(bufs))
        f.write(bytes(ops))


def test_tower_marks_trees_and_chain_traits_under_sanitizers(tmp_path):
    files = []
    for variant in EXPECTED:
        files.append(str(tmp_path / f"{variant}.prog"))
        _dump(files[-1], variant)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "tower_plan_host")
    cc = [hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Wno-unused-result", "-Wno-unused-value", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
          "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "tower_plan_host.hip"), "-o", exe]
    r = subprocess.run(cc, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    nm = subprocess.run(["nm", exe], capture_output=True, text=True, check=True).stdout
    assert "__asan_init" in nm and "__ubsan_handle" in nm  # the host code really is instrumented
    r = subprocess.run([exe, *files], capture_output=True, text=True, timeout=300)  # (LeakSanitizer runs at exit: a leak is a non-zero status)
    assert r.returncode == 0 and "tower plan host checks passed" in r.stdout, r.stdout + r.stderr


def test_the_tower_skip_is_a_statement_of_its_own_and_the_rule_names_no_op():
    net = open(os.path.join(ROOT, "head_detector_amd", "csrc", "net.hip")).read()
    rule = open(os.path.join(ROOT, "head_detector_amd", "csrc", "tower_plan.h")).read()
    assert net.count("op.tower) return VGH_OK;") == 1 and net.count("op.deferrable) return VGH_OK;") == 1
    code = "\n".join(line.split("//")[0] for line in rule.splitlines())
    assert "name" not in code.replace("namespace", "") and "flame" not in code.lower() and "stem" not in code.lower().replace("vgh_op_stem", "")
