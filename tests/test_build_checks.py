"""Build-time guard against silently mis-encoded device code.

ROCm 7.2's LLVM can select, for gfx950, an `s_mov_b64` of a 64-bit immediate
that the ISA cannot encode; the integrated assembler then keeps only the low 32
bits (tools/llvm_repro/).  build.check_device_asm re-assembles the compiler's
own text output with llvm-mc, which rejects such instructions, and build()
refuses a library whose device code fails it.

Also the inventory of compile-time switches (DESIGN.md "Build switches"): text
checks that no switch outside it is tested in csrc/ or defined by a variant."""
import os
import subprocess

import pytest

import noahmp_pkg  # noqa: F401
from noahmp_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPRO = os.path.join(ROOT, "tools", "llvm_repro", "s_mov_b64_literal.hip")


def _asm(tmp_path, name, flags):
    out = str(tmp_path / f"{name}.s")
    subprocess.run([build.HIPCC, "-O3", f"--offload-arch={build.ARCH}", "--offload-device-only",
                    "-S", "-o", out, REPRO, *flags], check=True, capture_output=True)
    return out


def test_asm_check_rejects_unencodable_literal(tmp_path):
    good = _asm(tmp_path, "default", [])
    build.check_device_asm([good], verbose=False)
    bad = _asm(tmp_path, "nomcse", ["-mllvm", "-disable-machine-cse"])
    with open(bad) as f:
        assert "s_mov_b64 s[0:1], 0x4049000000000000" in f.read()
    with pytest.raises(RuntimeError, match="unencodable"):
        build.check_device_asm([bad], verbose=False)


def test_shipped_library_built_with_asm_check():
    """build() runs the check by default (its signature), and the library in the
    tree is the one built from these sources."""
    import inspect
    assert inspect.signature(build.build).parameters["check_asm"].default is True
    assert build.built_hash() == build.source_hash()


# The whole inventory of compile-time switches of the product sources
# (DESIGN.md "Build switches"); NMP_DOM_* (vege_domain.h's constants) is a family.
SWITCHES = {"NMP_TU", "NMP_BUILD_HASH", "NMP_BLOCK",                       # structure
            "NMP_COUNT_FALLBACK", "NMP_DOM_*", "NMP_GM_BRANCHLESS",        # test-side
            "NMP_PHASE_TIMING", "NMP_TRUNC_RUNTIME", "NMP_WAVE_TIMING"}    # instruments


def _family(name):
    return "NMP_DOM_*" if name.startswith("NMP_DOM_") else name


def test_csrc_switch_inventory():
    """Every NMP_* name tested by a preprocessor conditional in csrc/ is on the
    allow-list, and every allow-listed switch still exists: a rejected
    experiment's switch does not come back into the product sources."""
    import re
    found = set()
    for name in sorted(os.listdir(build.CSRC)):
        with open(os.path.join(build.CSRC, name)) as f:
            for line in f:
                if re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b", line):
                    found.update(_family(n) for n in re.findall(r"\bNMP_[A-Z0-9_]+", line))
    assert found == SWITCHES


def test_variant_flags_name_real_switches():
    """Every -DNMP_X of tools/build_variants.py and of the probe library
    (__graft_entry__._build_probe_midloop) names a switch of the inventory: a
    variant that defines anything else would silently build the base library."""
    import re
    named = set()
    for path in (os.path.join(ROOT, "tools", "build_variants.py"),
                 os.path.join(ROOT, "__graft_entry__.py")):
        with open(path) as f:
            named.update(re.findall(r"-D(NMP_[A-Z0-9_]+)", f.read()))
    assert {"NMP_COUNT_FALLBACK", "NMP_DOM_TV_HI", "NMP_PHASE_TIMING"} <= named
    assert {_family(n) for n in named} <= SWITCHES
