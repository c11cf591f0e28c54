#!/bin/bash
# SQ counters of the checksum-verify kernels on the C2 batch (GPU box): what
# binds crc32_verify_kernel - LDS lookups, bank conflicts or memory.  Counter-only
# rocprofv3 passes over one configuration of tools/verify_cost.py, each under
# its own time limit; the first failure ends the script.
# usage: [OUT=dir] tools/verify_pmc.sh [kernel-name substring] [verify_cost config]
# (results under OUT, default prof_out/verifypmc in the repository)
set -o pipefail
R="$(cd "$(dirname "$0")/.." && pwd)"
K="${1:-crc32_verify_kernel}"
CFG="${2:-c2_gzip_4096}"
O="${OUT:-$R/prof_out/verifypmc}"
mkdir -p "$O"
cd /tmp && export TMPDIR=/tmp
i=0
for set in "SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_LDS SQ_ACTIVE_INST_LDS SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_INST_LDS SQ_INSTS_VALU" \
           "SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VMEM_RD SQ_WAVES SQ_ACTIVE_INST_VMEM SQ_INST_CYCLES_VMEM_RD"; do
  i=$((i+1))
  timeout -s KILL 300 rocprofv3 --pmc $set --output-format csv -d "$O/p$i" -o pmc -- \
    python3 "$R/tools/verify_cost.py" --child "$CFG" --steps 2 --warmup 1 \
    > "$O/p$i.log" 2>&1 || { echo "pass $i failed"; tail -5 "$O/p$i.log"; exit 1; }
done
K="$K" O="$O" python3 - <<'PY'
import csv, glob, os, collections, json
K = os.environ["K"]; O = os.environ["O"]
agg = collections.defaultdict(float); calls = collections.Counter()
for f in sorted(glob.glob(f"{O}/**/*counter_collection.csv", recursive=True)):
    for r in csv.DictReader(open(f)):
        if K not in r["Kernel_Name"]: continue
        agg[r["Counter_Name"]] += float(r["Counter_Value"])
        calls[r["Counter_Name"]] += 1
per = {k: v / max(1, calls[k]) for k, v in sorted(agg.items())}  # per launch
d = {}
if per.get("SQ_LDS_IDX_ACTIVE"):
    d["lds_bank_conflict_frac_of_lds_cycles"] = round(per.get("SQ_LDS_BANK_CONFLICT", 0) / per["SQ_LDS_IDX_ACTIVE"], 3)
if per.get("SQ_BUSY_CYCLES"):
    d["lds_active_cycles_per_busy_cycle"] = round(per.get("SQ_LDS_IDX_ACTIVE", 0) / per["SQ_BUSY_CYCLES"], 3)
if per.get("SQ_WAVE_CYCLES"):
    wc = per["SQ_WAVE_CYCLES"]
    d["wait_any_frac"] = round(per.get("SQ_WAIT_ANY", 0) / wc, 3)
    d["wait_inst_lds_frac"] = round(per.get("SQ_WAIT_INST_LDS", 0) / wc, 3)
    d["active_inst_any_frac"] = round(per.get("SQ_ACTIVE_INST_ANY", 0) / wc, 3)
out = {"kernel": K, "config": os.environ.get("CFG", ""), "launches": max(calls.values()) if calls else 0,
       "per_launch": per, "derived": d}
json.dump(out, open(f"{O}/summary.json", "w"), indent=1)
print(json.dumps(out, indent=1))
PY
