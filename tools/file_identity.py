#!/usr/bin/env python3
"""Output-file identity of two source trees, run by run (needs a GPU).

  python tools/file_identity.py emit WORKDIR LISTING    # run the cases with this tree
  python tools/file_identity.py record PARENT_LISTING PR_LISTING > profiles/.../file_identity.txt

`emit` runs, with the tree the script lies in, one small netCDF case
(tools/make_offline_case.py: 12 x 20 land points, 12 steps of 3600 s, output
every 3rd step, a restart every 4th -- step 4 lies inside an output interval):
a driver from the case's files over the 12 steps, then a second one from the
restart of step 4 to the end, writing beside the first.  The runs: accumulate x
extremes x state_out x regions, each off and on, in fp32; everything on in
fp64; and a synthetic run without a grid (npz files) with everything on, its
second driver loaded with load_restart.  The listing has one line per LDASOUT,
REGIONS and RESTART file: its path under WORKDIR and the SHA-256 of its bytes.
An .npz member carries the wall-clock time it was zipped at, so an .npz file is
hashed member by member instead: name, dtype, shape and bytes, in file order.

`record` compares two listings line by line; exit status 1 if any file differs.
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

EXTREMES = "FSH,TG,PRCP:max+tmax"
NML = """&NOAHMP_OFFLINE
  static_parameter_file = '{d}/geo_em.d01.nc'
  initialization_file = '{d}/init.nc'
  restart_file = '{d}/restart.nc'
  input_directory = '{d}/ldasin'
  input_frequency = '1 hour'
  output_directory = '{d}/ldasout'
  output_frequency = '3 hour'
  restart_directory = '{d}/restart'
  restart_frequency = '4 hour'
  start_year = 2000, start_month = 1, start_day = 1
  start_hour = 0  start_minute = 0  start_second = 0
  end_year = 2000 end_month = 1 end_day = 1 end_hour = 12 end_minute = 0 end_second = 0
  interval_seconds = 3600
  opt_veg = 1, opt_run = 1, opt_btr = 1, opt_rad = 1, opt_tub = 1, opt_can = 1
  opt_inf = 1, opt_tbot = 1, opt_snf = 1
/
"""


def runs():
    """(name, precision, driver options, with regions) of every run on the grid."""
    for acc in (False, True):
        for ext in (None, EXTREMES):
            for so in (None, "all"):
                for reg in (False, True):
                    name = "f32_acc%d_ext%d_state%d_reg%d" % (acc, ext is not None,
                                                              so is not None, reg)
                    yield name, 4, dict(accumulate=acc, extremes=ext, state_out=so), reg
    yield "f64_all", 8, dict(accumulate=True, extremes=EXTREMES, state_out="all"), True


def sha_file(path):
    h = hashlib.sha256()
    if path.endswith(".npz"):
        import numpy as np
        with np.load(path, allow_pickle=False) as z:
            for k in z.files:
                a = z[k]
                h.update(f"{k} {a.dtype.str} {a.shape}\n".encode())
                h.update(np.ascontiguousarray(a).tobytes())
    else:
        with open(path, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def emit(work, listing):
    import numpy as np
    import noahmp_pkg  # noqa: F401
    import make_offline_case
    from noahmp_amd import cases, config, driver, ncio, timeman
    from noahmp_amd.params import Params
    work = os.path.abspath(work)
    os.makedirs(work, exist_ok=True)
    nml = os.path.join(work, "case.nml")
    with open(nml, "w") as f:
        f.write(NML.format(d=work))
    make_offline_case.main([nml, "--ny", "12", "--nx", "20", "--kind", "mixed"])
    P = Params.builtin()
    grid, _, _ = ncio.read_static(config.Config(nml).constfile, P.as_dict(),
                                  config.Config(nml).begdatetime)
    regfile = os.path.join(work, "regions.nc")
    ncio.write_region_map(regfile, grid, (np.arange(grid.n) % 7) - 1)

    def dirs(cfg, name, part):
        cfg.outdir = os.path.join(work, name, part, "ldasout")
        cfg.resdir = os.path.join(work, name, part, "restart")
        return cfg

    for name, prec, kw, reg in runs():
        rkw = dict(regions=regfile) if reg else {}
        a = driver.OfflineDriver.from_files(dirs(config.Config(nml), name, "whole"),
                                            precision=prec, **kw, **rkw)
        a.run()
        a.engine.close()
        mid = os.path.join(work, name, "whole", "restart", "RESTART.2000010104_DOMAIN1.nc")
        b = driver.OfflineDriver.from_files(dirs(config.Config(nml), name, "resumed"), init=mid,
                                            precision=prec, **kw, **rkw)
        assert b.step_index == 4
        b.run()
        b.engine.close()
        print("ran", name, flush=True)
    # without a grid: npz output and restarts, the second driver loaded with load_restart
    name, kw = "f32_synthetic_all", dict(accumulate=True, extremes=EXTREMES, state_out="all")
    cfg = dirs(config.Config(nml), name, "whole")
    cols = cases.make_columns(300, "mixed", P.as_dict(), seed=3,
                              julian=timeman.julian(cfg.begdatetime))
    a = driver.OfflineDriver(cfg, cols, **kw)
    a.run()
    a.engine.close()
    b = driver.OfflineDriver(dirs(config.Config(nml), name, "resumed"), cols, **kw)
    b.load_restart(os.path.join(work, name, "whole", "restart", "RESTART.2000010104.r0.npz"))
    assert b.step_index == 4
    b.run()
    b.engine.close()
    print("ran", name, flush=True)
    lines = []
    for d, _, files in sorted(os.walk(work)):
        for fn in sorted(files):
            if "LDASOUT" in fn or "REGIONS" in fn or fn.startswith("RESTART"):
                p = os.path.join(d, fn)
                lines.append(f"{sha_file(p)}  {os.path.relpath(p, work)}")
    os.makedirs(os.path.dirname(os.path.abspath(listing)), exist_ok=True)
    with open(listing, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"{len(lines)} files listed in {listing}")


def record(parent, pr):
    def read(path):
        with open(path) as f:
            return dict(reversed(line.rstrip("\n").split("  ", 1)) for line in f if line.strip())
    a, b = read(parent), read(pr)
    same = 0
    for name in sorted(set(a) | set(b)):
        ok = a.get(name) == b.get(name)
        same += ok
        print(f"{'IDENTICAL' if ok else 'DIFFERENT'}  {name}\n"
              f"  parent {a.get(name, '(no such file)')}\n  pr     {b.get(name, '(no such file)')}")
    print(f"\n{same} of {len(set(a) | set(b))} files identical")
    return 0 if same == len(set(a) | set(b)) and a else 1


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "emit":
        emit(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 4 and sys.argv[1] == "record":
        sys.exit(record(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
