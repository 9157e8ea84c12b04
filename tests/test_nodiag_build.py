"""Build-side checks of the no-diagnostics step kernels (no GPU needed).

The fp32 unit of the engine library holds nine step kernels: the seven it had
(full and half occupancy x option sets 1, 2, 0 with `ref` math, and the
fast-math kernel) and the two compiled without the diagnostics, option sets 1
and 2 at full occupancy (sflx_kernel.hip kNoDiag: OS 1|4 and 2|4).
"""
import re
import shutil

import noahmp_pkg  # noqa: F401
from noahmp_amd import build

KERNEL = "_ZN3nmp16sflx_step_kernelIfLb%dELb%dELi%dEEEvPKNS_9DevParamsENS_5KArgsIT_EE"
SEVEN = {KERNEL % (1, small, os_) for small in (0, 1) for os_ in (0, 1, 2)} | {KERNEL % (0, 0, 0)}
NEW = {KERNEL % (1, 0, 5), KERNEL % (1, 0, 6)}


def test_library_holds_the_two_new_kernels_beside_the_seven():
    build.build(verbose=False)
    with open(build.DEFAULT_LIB_PATH, "rb") as f:
        data = f.read()
    found = {m.decode() for m in re.findall(rb"_ZN3nmp16sflx_step_kernelIf\w+", data)}
    assert found == SEVEN | NEW, sorted(found ^ (SEVEN | NEW))


def test_source_hash_follows_the_kernel_source(tmp_path, monkeypatch):
    """A library built before a change to the kernel source carries another
    hash than the sources', and lib.load() refuses it as stale."""
    import pytest
    from noahmp_amd import lib as lib_mod
    assert build.built_hash(build.DEFAULT_LIB_PATH) == build.source_hash()
    csrc = tmp_path / "csrc"
    shutil.copytree(build.CSRC, csrc)
    with open(csrc / "sflx_kernel.hip", "a") as f:
        f.write("// changed\n")
    monkeypatch.setattr(build, "CSRC", str(csrc))
    assert build.source_hash() != build.built_hash(build.DEFAULT_LIB_PATH)
    monkeypatch.setattr(build, "LIB_PATH", build.DEFAULT_LIB_PATH)
    monkeypatch.setattr(lib_mod, "_lib", None)
    with pytest.raises(RuntimeError, match="stale"):
        lib_mod.load()


def test_kernarg_check_covers_the_new_kernels(tmp_path):
    """check_kernarg_layout looks at every sflx_step_kernel of a unit, the new
    names included: KArgs at another offset than 8 in one of them is refused."""
    import pytest

    def meta(name, off2):
        return (f"  - .args:\n      - .offset: 0\n        .size: 8\n      - .offset: {off2}\n"
                f"        .size: 240\n        .value_kind: by_value\n    .name: {name}\n")
    good, bad = tmp_path / "good.s", tmp_path / "bad.s"
    good.write_text("".join(meta(n, 8) for n in sorted(SEVEN | NEW)))
    bad.write_text("".join(meta(n, 16 if n in NEW else 8) for n in sorted(SEVEN | NEW)))
    build.check_kernarg_layout([str(good)])
    with pytest.raises(RuntimeError, match="KArgs not at byte offset 8") as e:
        build.check_kernarg_layout([str(bad)])
    assert all(n in str(e.value) for n in NEW)
