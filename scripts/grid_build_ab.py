"""A/B of the grid build between two libraries (PCR_LIB_PATH): bench.py's own `setup` figures on the 120k pair and its `batch256`
compat / tight figures, each library in a fresh process, alternately, RUNS times each.

  python scripts/grid_build_ab.py --parent scripts/bin/libpcr_parent.so --out profiles/grid_build_ab.json [--runs 5] [--what "the change"]
  python scripts/grid_build_ab.py --one            one run of the library in PCR_LIB_PATH (default: the built one), a JSON line
  python scripts/grid_build_ab.py --prof           the build kernels a few times, for rocprofv3 --kernel-trace --stats
  python scripts/grid_build_ab.py --fold-stats PARENT_kernel_stats.csv NEW_kernel_stats.csv --out profiles/grid_build_kernel_stats.csv

Margin (per figure, lower is better): median(new) - median(parent) <= max(parent) - min(parent) of the same session.  bench.py's bit
check of the fused batch against the per-pair path is recorded per run and printed beside the speed verdict.  A child
process that fails ends the session: nothing more is started on the device."""
import argparse, csv, importlib, json, os, statistics, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIGURES = ("setup.target_upload_ms", "setup.index_build_ms", "setup.source_upload_ms", "setup.prepare_ms",
           "setup.compat_registration_on_built_index_ms", "batch256.compat.seconds", "batch256.tight.seconds")
JUDGED = ("setup.index_build_ms", "setup.prepare_ms", "batch256.compat.seconds", "batch256.tight.seconds")
KERNELS = ("morton_keys_var_kernel", "gather_count_kernel", "init_pools_kernel", "insert_cells_var_kernel", "insert_blocks_var_kernel",
           "batch_keys_kernel", "batch_count_kernel", "batch_plan_kernel", "batch_init_tables_kernel", "batch_insert_cells_kernel",
           "batch_insert_blocks_kernel")


def one():
    bench = importlib.import_module("bench")
    pkg = importlib.import_module("point-cloud-process_amd")
    ctx = pkg.Context(0)
    src, tgt, _ = pkg.synthetic.perturbed_pair(bench.N_POINTS, seed=0)
    bench.device_warmup(pkg, ctx, src, tgt, 0.0)
    setup = bench.setup_leg(pkg, ctx, src, tgt, 0.0)
    b = bench.batch_leg(pkg, None, None, 0, 1, 0, "cuda:0", 8)
    row = {"setup." + k: v for k, v in setup.items() if k != "note"}
    for tag in ("compat", "tight"):
        row[f"batch256.{tag}.seconds"] = b[tag]["seconds"]
        row[f"batch256.{tag}.runs_s"] = b[tag]["runs_s"]
        row[f"batch256.{tag}.bitwise_equal_to_per_pair_path"] = b[tag]["per_pair_path"]["results_bitwise_equal_to_fused"]
    print("AB " + json.dumps(row), flush=True)


def prof():
    pkg = importlib.import_module("point-cloud-process_amd")
    batch = importlib.import_module("point-cloud-process_amd.batch")
    ctx = pkg.default_context()
    src, tgt, _ = pkg.synthetic.perturbed_pair(120000, seed=0)
    dt = pkg.DeviceCloud.upload(tgt, ctx)
    for cell in (0.0, 0.01):   # 32-bit keys (30 varying bits at the automatic cell), 64-bit keys
        for _ in range(10):
            pkg.TargetIndex(dt, cell=cell, ctx=ctx).free()
    pairs = [(s, t, None) for s, t, _ in pkg.synthetic.registration_batch_6f(64, 20000, seed=1000)]
    for _ in range(3):
        batch.native_register_share(pairs, device=0, streams=1)
    print("prof done", flush=True)


def fold_stats(parent_csv, new_csv, out):
    rows = []
    for lib, path in (("parent", parent_csv), ("new", new_csv)):
        for r in csv.DictReader(open(path)):
            name = r["Name"].split("(")[0].replace("void ", "")
            if name.split("<")[0] in KERNELS:
                rows.append([lib, name, r["Calls"], r["AverageNs"], r["MinNs"], r["MaxNs"]])
    rows.sort(key=lambda r: (r[1], r[0] != "parent"))
    with open(out, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["library", "kernel", "calls", "average_ns", "min_ns", "max_ns"])
        w.writerows(rows)
    for r in rows:
        print("%-8s %-48s calls %5s avg %9.1f us" % (r[0], r[1][:48], r[2], float(r[3]) / 1e3))


def session(parent, runs, out, timeout, what):
    libs = (("parent", os.path.abspath(parent)), ("new", os.path.join(ROOT, "point-cloud-process_amd", "libpcr.so")))
    got = {"parent": [], "new": []}
    for r in range(runs):
        for tag, path in libs:
            env = dict(os.environ, PCR_LIB_PATH=path)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one"], env=env, capture_output=True, text=True, timeout=timeout)
            line = next((l for l in p.stdout.splitlines() if l.startswith("AB ")), None)
            if p.returncode != 0 or line is None:
                print(p.stdout[-2000:], p.stderr[-2000:])
                sys.exit(f"run {r} of the {tag} library failed (exit {p.returncode}): session ended")
            got[tag].append(json.loads(line[3:]))
            print(tag, r, {k: round(got[tag][-1][k], 5) for k in FIGURES}, flush=True)
    res = {"what": f"A/B of {what}: bench.py's setup figures (ms, best of "
                   "10, 120 000-point pair) and batch256 seconds (best of 8, 256 x 20 000-point pairs, 8 contexts) for the parent commit's library "
                   f"and the new one, {runs} fresh processes each, alternately (parent, new, ...) in one session on one MI355X; margin = the "
                   "parent's own max - min; inside = median(new) - median(parent) <= margin",
           "runs": got, "figures": {}}
    for k in FIGURES:
        a, b = [x[k] for x in got["parent"]], [x[k] for x in got["new"]]
        margin = max(a) - min(a)
        res["figures"][k] = {"parent": a, "new": b, "parent_median": statistics.median(a), "new_median": statistics.median(b), "margin": margin,
                             "judged": k in JUDGED, "inside": statistics.median(b) - statistics.median(a) <= margin}
    # bench.py's own bit check of the fused batch against the per-pair path (the last of its 8 fused runs against the last per-pair run):
    # runs of each library in which it did NOT hold.  Not a figure of the speed verdict; never to be passed over in silence.
    res["runs_not_bitwise_equal_to_per_pair_path"] = {f"{lib}.{t}": [i for i, x in enumerate(v) if not x[f"batch256.{t}.bitwise_equal_to_per_pair_path"]]
                                                      for lib, v in got.items() for t in ("compat", "tight")}
    res["verdict"] = "met" if all(f["inside"] for f in res["figures"].values() if f["judged"]) else "not met"
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    for k, f_ in res["figures"].items():
        print("%-48s parent %.5f new %.5f margin %.5f %s%s" % (k, f_["parent_median"], f_["new_median"], f_["margin"], "inside" if f_["inside"] else "OUTSIDE",
                                                                "" if f_["judged"] else " (not judged)"))
    print("speed verdict:", res["verdict"])
    for k, v in res["runs_not_bitwise_equal_to_per_pair_path"].items():
        print("bench.py's results_bitwise_equal_to_fused, %-14s %s" % (k, "true in every run" if not v else "FALSE in runs %s of %d" % (v, runs)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--prof", action="store_true")
    ap.add_argument("--fold-stats", nargs=2, metavar=("PARENT_CSV", "NEW_CSV"))
    ap.add_argument("--parent", default=os.path.join(ROOT, "scripts", "bin", "libpcr_parent.so"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--timeout", type=float, default=240.0, help="seconds per child process")
    ap.add_argument("--out", default=None)
    ap.add_argument("--what", default="the grid-build refactor (one copy of the table build, csrc/pcr_grid_build_dev.h)", help="the change under test, for the record's first line")
    a = ap.parse_args()
    if a.one:
        one()
    elif a.prof:
        prof()
    elif a.fold_stats:
        fold_stats(a.fold_stats[0], a.fold_stats[1], a.out or os.path.join(ROOT, "profiles", "grid_build_kernel_stats.csv"))
    else:
        session(a.parent, a.runs, a.out or os.path.join(ROOT, "profiles", "grid_build_ab.json"), a.timeout, a.what)
