#!/bin/bash
# HBM traffic of the three bf16 update kernels with the learner's workspaces in panel order: `--pmc FETCH_SIZE` and `--pmc WRITE_SIZE`
# in separate runs of tools/panel_order_probe.py (the actor's update chunk at 2^22 rows), against the algorithmic bytes per row.
#   [OUT_DIR=dir] bash tools/panel_order_pmc.sh [config]   -> $OUT_DIR/panel_order_pmc_<config>.json   (config: all_panel | dz_panel | row_major;
#   OUT_DIR defaults to build/profiles, which git ignores)
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
CFG=${1:-all_panel}
OUT_DIR=${OUT_DIR:-$R/build/profiles}
OUT=$OUT_DIR/pmc_$CFG
rm -rf $OUT && mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
for c in FETCH_SIZE WRITE_SIZE; do
  timeout -k 10 300 rocprofv3 --pmc $c --output-format csv -d $OUT/$c -- python3 $R/tools/panel_order_probe.py --configs $CFG --nets 4 --passes 1 --iters 3 > $OUT/$c.log 2>&1
done
python3 - "$OUT" "$CFG" > $OUT_DIR/panel_order_pmc_$CFG.json <<'PY'
import csv, glob, json, sys, collections
out, cfg = sys.argv[1], sys.argv[2]
probe = json.loads([l for l in open(out + "/FETCH_SIZE.log") if l.startswith("{")][-1])
fam_of = {"mlp_fwd_chain_kernel": "fwd", "mlp_bwd_chain_kernel": "bwd", "dw_kernel": "dw"}
acc = collections.defaultdict(lambda: collections.defaultdict(list))
names = {}
for f in glob.glob(out + "/*/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        for pat, fam in fam_of.items():
            if pat in r["Kernel_Name"]:
                acc[fam][r["Counter_Name"]].append(float(r["Counter_Value"]))
                names[fam] = r["Kernel_Name"].split("(")[0]
res = {"command": "rocprofv3 --pmc FETCH_SIZE|WRITE_SIZE (separate passes) -- python3 tools/panel_order_probe.py --configs %s --nets 4 --passes 1 --iters 3" % cfg,
       "rows": probe["rows"], "config": cfg, "kernels": {}}
for fam, a in acc.items():
    fetch, write = a["FETCH_SIZE"], a["WRITE_SIZE"]
    rd, wr = 2 * 1024 * sum(fetch) / len(fetch), 1024 * sum(write) / len(write)     # (KiB; read bytes = 2 x FETCH_SIZE on gfx950: profiles/README.md)
    alg = probe["rows"] * probe["bytes_per_row"][fam]
    res["kernels"][fam] = {"kernel": names[fam], "launches_fetch": len(fetch), "launches_write": len(write), "read_bytes_per_launch": rd,
                           "write_bytes_per_launch": wr, "traffic_bytes_per_launch": rd + wr, "algorithmic_bytes_per_launch": alg,
                           "traffic_over_algorithmic": (rd + wr) / alg}
json.dump(res, sys.stdout, indent=1)
PY
rm -rf $OUT
echo done
