"""csrc/glibc_math.h (the kernel's "ref" math) vs the host glibc float libm.

The header is __host__ __device__; here it is compiled for the host with the
same -ffp-contract=off -- by g++ and by ROCm's clang++, the host compiler of
the GPU math test's reference (tests/test_gpu_math.py) -- and compared bit for
bit against libm.  Default run:
every 61st of the 2^32 float patterns per univariate function, powf on a
stride x 30 exponents + random pairs.  NMP_EXHAUSTIVE=1 checks all 2^32
(each function ~6 s on 8 cores; the committed design claims were made with
that run: 0 mismatches for every function, powf 0 of 2.6e10).
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "glibc_math_check.cpp")
FUNCS = ["expf", "exp2f", "logf", "expm1f", "tanhf", "atanf", "log10f", "acosf", "cosf", "tanf"]


def _compilers():
    """g++, and ROCm's clang++ (next to build.LLVM_MC): hipcc's host compiler,
    whose compilation of the header is the reference of tests/test_gpu_math.py.
    Same flags; -fopenmp only where its OpenMP runtime is present."""
    import noahmp_pkg  # noqa: F401
    from noahmp_amd import build
    llvm_bin = os.path.dirname(build.LLVM_MC)
    clang = os.path.join(llvm_bin, "clang++")
    libdir = os.path.join(os.path.dirname(llvm_bin), "lib")
    omp = ["-fopenmp", f"-Wl,-rpath,{libdir}"] if os.path.exists(
        os.path.join(libdir, "libomp.so")) else []
    return {"g++": ["g++", "-fopenmp"], "clang++": [clang, *omp]}


@pytest.fixture(scope="module",
                params=[("g++", 0), ("g++", 1), ("clang++", 0), ("clang++", 1)],
                ids=["branches", "branchless", "clang-branches", "clang-branchless"])
def checker(request, tmp_path_factory):
    """The header as compiled by default and with NMP_GM_BRANCHLESS=1 (the
    special-case exits of expf/logf as selects), by g++ and by ROCm's clang++."""
    cc, branchless = request.param
    cmd = _compilers()[cc]
    if not (os.path.exists(cmd[0]) or cc == "g++"):
        pytest.fail(f"{cmd[0]} missing: the GPU math test's host reference cannot be tied to libm")
    exe = str(tmp_path_factory.mktemp("gm") / "glibc_math_check")
    subprocess.run([*cmd, "-O2", "-ffp-contract=off", "-std=c++17",
                    f"-DNMP_GM_BRANCHLESS={branchless}",
                    "-I", os.path.join(ROOT, "noahmp-1_amd", "csrc"), "-o", exe, SRC, "-lm"],
                   check=True)
    return exe


def _stride(default):
    return "1" if os.environ.get("NMP_EXHAUSTIVE") == "1" else str(default)


@pytest.mark.parametrize("fn", FUNCS)
def test_bit_exact_vs_host_libm(checker, fn):
    r = subprocess.run([checker, fn, _stride(61)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and " mismatches 0 of " in r.stdout, r.stdout + r.stderr


def test_powf_bit_exact_vs_host_libm(checker):
    r = subprocess.run([checker, "powf", _stride(997)], capture_output=True, text=True,
                       timeout=1200)
    assert r.returncode == 0 and " mismatches 0 of " in r.stdout, r.stdout + r.stderr


def test_powf_pair_bit_exact_vs_host_libm(checker):
    """gm::powf_pair (one log2 of the base for two exponents) == two host powf."""
    r = subprocess.run([checker, "powf_pair", _stride(997)], capture_output=True, text=True,
                       timeout=1200)
    assert r.returncode == 0 and " mismatches 0 of " in r.stdout, r.stdout + r.stderr
