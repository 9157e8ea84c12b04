"""The sign half of the short-division range proof (tools/div_proof.py): a site
that calls DivFast32::divn (no v_div_fixup_f32) needs a numerator that is never
-0, the proof tracks the sign of every numerator's zero, and the kernel calls
divn exactly at the sites the proof declares fix-up-free."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROOF = os.path.join(ROOT, "tools", "div_proof.py")
CSRC = os.path.join(ROOT, "noahmp-1_amd", "csrc")
ROW = re.compile(r"^(?P<name>\S.*?)\s+(?P<ref>:\d\S*(?: \(once per loop\))?|atanf)\s+.*\s"
                 r"(?P<ok>yes|NO)\s+(?P<sign>[-+]+(?: 0:[-+]+0)?)\s+(?P<neg0>never|maybe)\s+"
                 r"(?P<fix>dropped|kept)\b")


def _rows(stdout):
    rows = {}
    for ln in stdout.splitlines():
        m = ROW.match(ln)
        if m:
            rows[m.group("name")] = m.groupdict()
    return rows


def test_proof_passes_and_declares_every_site():
    r = subprocess.run([sys.executable, PROOF], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = _rows(r.stdout)
    assert len(rows) >= 55, sorted(rows)
    kept = sorted(n for n, v in rows.items() if v["fix"] == "kept")
    # EVC and TR meet -0 (a dry canopy under dew) and keep the fix-up; nothing else does
    assert kept == ["EVC = FVEG*RHOAIR*CPAIR*CEW*(ESTV-EAH) / GAMMAV",
                    "TR = FVEG*RHOAIR*CPAIR*CTW*(ESTV-EAH) / GAMMAV"], kept
    for n in kept:
        assert rows[n]["neg0"] == "maybe" and rows[n]["ok"] == "yes"
    free = [n for n, v in rows.items() if v["fix"] == "dropped"]
    assert all(rows[n]["neg0"] == "never" and rows[n]["ok"] == "yes" for n in free)
    m = re.search(r"^(\d+) sites fix-up-free, none with a numerator that can be -0$", r.stdout, re.M)
    assert m and int(m.group(1)) == len(free)
    # the groups the kernel converts: the canopy loop's body, sfcdif1 and ragrb,
    # the bare loop, the bisection, the soil sub-steps, atanf_ge1
    for n in ("CTR = (1-BEA)*CTW*RHOAIR*CPAIR / GAMMAV", "DTV = B / A", "MOL = -FV**3 / TMP1",
              "RAHG = TMPRAH2 / KH", "bare: DTG = B / A", "stomata: R2 = C / Q",
              "soil: RHSTT = WFLUX / (-DENOM)", "libm: ATAN's NUM / DEN"):
        assert n in free, n


def test_proof_refuses_evc_declared_fixup_free(tmp_path):
    """The proof reads the header, so this runs a copy of the tree's two files
    with EVC's declaration dropped: CEW = +0 times a negative ESTV - EAH is -0."""
    tools = tmp_path / "tools"
    csrc = tmp_path / "noahmp-1_amd" / "csrc"
    tools.mkdir()
    csrc.mkdir(parents=True)
    (csrc / "vege_domain.h").write_text(open(os.path.join(CSRC, "vege_domain.h")).read())
    src = open(PROOF).read()
    old = '":2842", "-0 under dew on a dry canopy", fix=True)'
    assert src.count(old) == 1
    (tools / "div_proof.py").write_text(src.replace(old, '":2842", "-0 under dew on a dry canopy")'))
    r = subprocess.run([sys.executable, str(tools / "div_proof.py")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 1 and "FAILED" in r.stdout, r.stdout[-1500:]
    failed = r.stdout[r.stdout.index("FAILED"):]
    assert "EVC = " in failed and "TR = " not in failed and "CTR" not in failed, failed
    evc = _rows(r.stdout)["EVC = FVEG*RHOAIR*CPAIR*CEW*(ESTV-EAH) / GAMMAV"]
    assert evc["ok"] == "NO" and evc["neg0"] == "maybe" and evc["fix"] == "dropped"


def test_kernel_calls_div_only_at_the_sites_that_keep_the_fixup():
    """DivFast32::div is left at EVC and TR; every other quotient of the
    policies goes through divn, and the "0 or in range" numerators are tested
    as the bit pattern of +0."""
    src = open(os.path.join(CSRC, "sflx_kernel.hip")).read()
    div_calls = re.findall(r"^.*\b\w+\.div\(.*$", src, re.M)
    assert len(div_calls) == 2, div_calls
    assert div_calls[0].strip().startswith("evc = d.div(") and "(estv - c.eah)" in div_calls[0]
    assert div_calls[1].strip() == "tr = d.div(tr_n, rgammav);"
    assert not re.search(r"\b\w+\.divk\(", src)
    # 49 call sites in the source (the proof's table folds a few: AI/CI/BI, the
    # two DSMDZ branches): a change here means a new row in tools/div_proof.py
    assert len(re.findall(r"\b\w+\.divn\(", src)) == 49
    assert "is_pzero(x) || in(x, lo, hi)" in src            # ZPD, LAISUNE, LAISHAE, FWET
    assert "is_pzero(c.eah)" in src and "is_pzero(sp.fnf)" in src
    assert "const bool in = is_pzero(a) ||" in src          # the soil sub-steps' numerators
    math = open(os.path.join(CSRC, "sflx_math.h")).read()
    assert "return d.divn(a, d.rec(b));" in math             # atanf_ge1's quotient
