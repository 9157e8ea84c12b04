"""The libm sites of the range proof (tools/div_proof.py) hold: every argument
of the in-range cores the Newton loops call under DivFast32 lies inside its
core's interval, for the windows csrc/vege_domain.h defines (the one copy of
the numbers), and the static bounds lie inside those windows."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "noahmp-1_amd", "csrc", "vege_domain.h")
SITES = ["(MOZ) TMP1 = (1 - 16 MOZ)**0.25", "(MOZ) LOG((1 + TMP1**2) / 2)",
         "(MOZ) LOG((1 + TMP1) / 2)", "(MOZ) ATAN(TMP1)",
         "(MOZ2) TMP1 = (1 - 16 MOZ2)**0.25", "(MOZ2) LOG((1 + TMP1**2) / 2)",
         "(MOZ2) LOG((1 + TMP1) / 2)", "(MOZ2) ATAN(TMP1)",
         "FHGNEW = (1 - 15 MOZG)**(-0.25)", "EXP(-CWPC*Z0HG / HCAN)",
         "EXP(-CWPC*(Z0H+ZPD) / HCAN)", "EXP(CWPC)", "EXP(-CWPC / 2)", "ATAN's NUM / DEN"]


def _proof(env=None):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "div_proof.py")],
                          capture_output=True, text=True, timeout=300, env=env)


def test_every_libm_site_is_inside_its_core_interval():
    r = _proof()
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "all 13 libm sites inside their cores' intervals" in r.stdout
    for s in SITES:
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("libm: " + s + " ")]
        assert len(line) == 1 and "  yes" in line[0] and "  NO" not in line[0], (s, line)


def test_header_windows_are_the_ones_the_proof_used():
    hdr = open(HDR).read()
    D = {m.group(1): float(m.group(2))
         for m in re.finditer(r"#define NMP_DOM_(\w+) ([-+0-9.eE]+)", hdr)}
    assert D["MOZ_LO"] < 0 and D["MOZG_LO"] < 0
    m = re.search(r"libm windows: MOZ_LO = (\S+), MOZG_LO = (\S+) \(static: \|MOZ\| <= (\S+), "
                  r"\|MOZ2\| <= (\S+), \|MOZG\| <= (\S+)\)", _proof().stdout)
    assert m, "the proof does not print its windows"
    assert float(m.group(1)) == D["MOZ_LO"] and float(m.group(2)) == D["MOZG_LO"]
    # the shipped windows lie outside what the static domain allows: a lane
    # inside that domain never leaves through them
    assert max(float(m.group(3)), float(m.group(4))) < -D["MOZ_LO"]
    assert float(m.group(5)) < -D["MOZG_LO"]
    # the kernel folds exactly these names into the lanes' `ok`
    src = open(os.path.join(ROOT, "noahmp-1_amd", "csrc", "sflx_kernel.hip")).read()
    assert "moz >= (T)NMP_DOM_MOZ_LO" in src and "moz2 >= (T)NMP_DOM_MOZ_LO" in src
    assert "mozg >= (T)NMP_DOM_MOZG_LO" in src
    for bit in (32, 33, 34):
        assert re.search(rf"NMP_DOM\(ok, {bit}, ", src)


def test_proof_refuses_a_window_too_wide_for_atanf(tmp_path):
    """2^25 is atanf_ge1's upper end: (1 + 16 * 1e30)**0.25 = 2e7 is inside,
    a MOZ window of -1e32 (6.3e7 > 2^25) is not.  The proof reads the header,
    so this runs it on a copy of the tree's two files with the constant changed."""
    tools = tmp_path / "tools"
    csrc = tmp_path / "noahmp-1_amd" / "csrc"
    tools.mkdir()
    csrc.mkdir(parents=True)
    (tools / "div_proof.py").write_text(open(os.path.join(ROOT, "tools", "div_proof.py")).read())
    hdr = open(HDR).read()
    assert hdr.count("#define NMP_DOM_MOZ_LO -1.0e16") == 1
    (csrc / "vege_domain.h").write_text(hdr.replace("#define NMP_DOM_MOZ_LO -1.0e16",
                                                    "#define NMP_DOM_MOZ_LO -1.0e32"))
    r = subprocess.run([sys.executable, str(tools / "div_proof.py")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 1 and "FAILED" in r.stdout and "ATAN(TMP1)" in r.stdout, r.stdout[-1500:]
