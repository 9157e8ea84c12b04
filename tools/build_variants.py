"""Build tuning variants of the engine library into noahmp-1_amd/lib/variants/."""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import noahmp_pkg  # noqa: E402,F401
from noahmp_amd import build  # noqa: E402

VARIANTS = {
    "base": (),
    # measurement instruments and test-side switches (DESIGN.md "Build switches")
    "phase": ("-DNMP_PHASE_TIMING",),
    # per-phase truncation at a run-time mark (tools/phase_counters.sh)
    "trunc": ("-DNMP_TRUNC_RUNTIME",),
    # per-wave start/end records (tools/wave_timeline.py)
    "wt": ("-DNMP_WAVE_TIMING",),
    # the default build plus a device counter of lanes that re-ran the canopy
    # loop with IEEE division (nmp_debug_fallback_count)
    "fbcount": {"f32": ["-DNMP_COUNT_FALLBACK"]},
    # the libm calls outside the Newton loops (sflx_math.h MthGuard32) with their
    # intervals narrowed: most waves run the full functions (tests/probe_libm_outloop.py)
    "probe_libm_outloop": {"f32": ["-DNMP_COUNT_FALLBACK", "-DNMP_DOM_EXPF_HI=-1.0e30f",
                                   "-DNMP_DOM_LOGF_LO=1.0e30f", "-DNMP_DOM_POWF_LO=1.0e30f"]},
    "gmbl": ("-DNMP_GM_BRANCHLESS=1",),
    "b128": ("-DNMP_BLOCK=128",),
    "b64": ("-DNMP_BLOCK=64",),
    "b512": ("-DNMP_BLOCK=512",),
    # compiler flags, every translation unit
    "s_maxilp": ("-mllvm", "-amdgpu-sched-strategy=max-ilp"),
    "s_memclause": ("-mllvm", "-amdgpu-sched-strategy=max-memory-clause"),
    "s_itminreg": ("-mllvm", "-amdgpu-sched-strategy=iterative-minreg"),
    "s_nomisched": ("-mllvm", "-enable-misched=false"),
    "s_postup": ("-mllvm", "-misched-postra-direction=bottomup"),
    "mlicm": ("-mllvm", "-disable-machine-licm=false"),
    "split_speed": ("-mllvm", "-split-spill-mode=speed"),
    "split_size": ("-mllvm", "-split-spill-mode=size"),
    "rptrack": ("-mllvm", "-amdgpu-use-amdgpu-trackers"),
    "dce_ra": ("-mllvm", "-amdgpu-dce-in-ra"),
    "nounclust": ("-mllvm", "-amdgpu-disable-unclustered-high-rp-reschedule"),
    "relaxocc": ("-mllvm", "-amdgpu-schedule-relaxed-occupancy"),
    # timing probe only (NOT bit-exact): upper bound of what faster division
    # / sqrt sequences could save
    "nocrdiv": ("-fno-hip-fp32-correctly-rounded-divide-sqrt",),
    "noslp": ("-fno-slp-vectorize",),
    # the SLP vectorizer back on (the base flags' -fno-slp-vectorize overridden)
    "slp": ("-fslp-vectorize",),
    "nolpre": ("-mllvm", "-enable-load-pre=false"),
    "nopre": ("-mllvm", "-enable-pre=false"),
    "nounroll": ("-fno-unroll-loops",),
    "nopostmis": ("-mllvm", "-enable-post-misched=false"),
    "nosink": ("-mllvm", "-simplifycfg-sink-common=false"),
    "nohoist": ("-mllvm", "-simplifycfg-hoist-common=false"),
    "phifold8": ("-mllvm", "-two-entry-phi-node-folding-threshold=8"),
    "exhaust": ("-mllvm", "-exhaustive-register-search"),
    "defer": ("-mllvm", "-enable-deferred-spilling"),
    "nomcse": ("-mllvm", "-disable-machine-cse"),
    "notaildup": ("-mllvm", "-disable-tail-duplicate", "-mllvm", "-disable-early-taildup"),
    "gvnsink": ("-mllvm", "-enable-gvn-sink"),
    "nolsv": ("-mllvm", "-amdgpu-load-store-vectorizer=false"),
    "gcprio": ("-mllvm", "-greedy-regclass-priority-trumps-globalness=true"),
    "o2": ("-O2",),
    # fp64 translation unit flags (the fp32 kernels unchanged)
    "f64ieee": {"f64": []},
    "f64afn": {"f64": ["-freciprocal-math", "-fapprox-func"]},
    # the fp64 translation unit alone without MachineCSE
    "nomcse64": {"f64": ["-mllvm", "-disable-machine-cse"]},
    # the fp64 small kernels without MachineLICM (the build before the split)
    "f64s_nolicm": {"f64s": ["-mllvm", "-disable-machine-licm"]},
    # fp32 translation unit only
    "notaildup32": {"f32": ["-mllvm", "-disable-tail-duplicate", "-mllvm", "-disable-early-taildup"]},
    "nosink32": {"f32": ["-mllvm", "-simplifycfg-sink-common=false"]},
    "phifold1_32": {"f32": ["-mllvm", "-two-entry-phi-node-folding-threshold=1"]},
    "specoff32": {"f32": ["-mllvm", "-speculate-one-expensive-inst=false"]},
    "maxilp32": {"f32": ["-mllvm", "-amdgpu-sched-strategy=max-ilp"]},
    "exhaust32": {"f32": ["-mllvm", "-exhaustive-register-search"]},
    "gcprio32": {"f32": ["-mllvm", "-greedy-regclass-priority-trumps-globalness=true"]},
    "nopostmis32": {"f32": ["-mllvm", "-enable-post-misched=false"]},
    "s_ilp": {"f32": ["-mllvm", "-amdgpu-sched-strategy=max-ilp"]},
    "s_itilp": {"f32": ["-mllvm", "-amdgpu-sched-strategy=iterative-ilp"]},
    "s_memcl": {"f32": ["-mllvm", "-amdgpu-sched-strategy=max-memory-clause"]},
    # base flags re-checked once the spills were gone: MachineLICM and GVN-PRE
    # back on ("drop": flag pairs removed from build.FLAGS)
    "licm": {"drop": [("-mllvm", "-disable-machine-licm")]},
    "pre": {"drop": [("-mllvm", "-enable-pre=false")]},
}
if __name__ == "__main__":
    names = sys.argv[1:] or list(VARIANTS)
    vdir = os.path.join(build.LIB_DIR, "variants")
    base_flags = list(build.FLAGS)

    def drop(flags, seqs):
        out, i = [], 0
        while i < len(flags):
            for q in seqs:
                if tuple(flags[i:i + len(q)]) == tuple(q):
                    i += len(q)
                    break
            else:
                out.append(flags[i])
                i += 1
        return out

    def one(n):
        v = VARIANTS[n]
        if isinstance(v, dict) and "drop" in v:  # run alone: build.FLAGS patched
            build.FLAGS = drop(base_flags, v["drop"])
            sf = {k: drop(f, v["drop"]) for k, f in build.SOURCE_FLAGS.items()}
            try:
                return build.build(force=True, verbose=False, out=os.path.join(vdir, f"lib_{n}.so"),
                                   source_flags=sf)
            finally:
                build.FLAGS = base_flags
        if isinstance(v, dict):  # per-source flags: {"extra": (...), "f64": [...]}
            sf = dict(build.SOURCE_FLAGS)
            if "f64" in v:
                sf["sflx_kernel_f64.hip"] = list(sf["sflx_kernel_f64.hip"]) + list(v["f64"])
            if "f64s" in v:  # extra flags for the fp64 small-kernel unit only
                sf["sflx_kernel_f64s.hip"] = list(sf["sflx_kernel_f64s.hip"]) + list(v["f64s"])
            if "f32" in v:  # extra flags for the fp32 translation unit only
                sf["sflx_kernel.hip"] = list(sf["sflx_kernel.hip"]) + list(v["f32"])
            return build.build(force=True, verbose=False, out=os.path.join(vdir, f"lib_{n}.so"),
                               extra=tuple(v.get("extra", ())), source_flags=sf,
                               check_asm=not n.startswith("nomcse"))
        return build.build(force=True, verbose=False, out=os.path.join(vdir, f"lib_{n}.so"), extra=v,
                           check_asm=not n.startswith("nomcse"))
    solo = [n for n in names if isinstance(VARIANTS[n], dict) and "drop" in VARIANTS[n]]
    with ThreadPoolExecutor(2) as ex:
        list(ex.map(one, [n for n in names if n not in solo]))
    for n in solo:
        one(n)
    print("built", names)
