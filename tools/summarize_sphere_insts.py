"""Per-kernel SQ instruction counters from rocprofv3's counter_collection.csv files, in the format of profiles/rNN_sq_counters.json.

    python tools/summarize_sphere_insts.py OUT.json COMMIT DIR [DIR ...]

DIR: the -d directories of passes such as
    SHR_BENCH_SKIP_TRAIN=1 rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU --output-format csv -d DIR -o bench -- \
        python bench.py --full --no-cpu-baseline
Only this project's sphere kernels are kept (the counters this file exists for: instructions per wave of the raster
kernels); a kernel seen at several problem sizes is split by grid size; COMMIT is recorded as given."""
import collections
import csv
import glob
import json
import os
import sys


def main():
    out_path, commit, dirs = sys.argv[1], sys.argv[2], sys.argv[3:]
    sq = collections.defaultdict(lambda: collections.defaultdict(list))
    for d in dirs:
        for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            with open(f) as fh:
                for r in csv.DictReader(fh):
                    k = r["Kernel_Name"].split("(")[0].replace("void ", "")
                    if "shr::sphere_" not in k:
                        continue
                    key = k + " grid=" + r["Grid_Size"] if "Grid_Size" in r else k
                    sq[key][r["Counter_Name"]].append(float(r["Counter_Value"]))
    out = {}
    for k, cs in sorted(sq.items()):
        m = {c: round(sum(v) / len(v), 1) for c, v in cs.items()}
        d = {"launches_seen": max(len(v) for v in cs.values()), "counters_mean_per_launch": m}
        if m.get("SQ_WAVES"):
            d["per_wave"] = {"VALU_instructions": round(m.get("SQ_INSTS_VALU", 0) / m["SQ_WAVES"], 1),
                             "SALU_instructions": round(m.get("SQ_INSTS_SALU", 0) / m["SQ_WAVES"], 1)}
        out[k] = d
    out["_commit"] = commit
    out["_note"] = ("rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU (one pass, no tracing beside it) on bench.py --full "
                    "--no-cpu-baseline with SHR_BENCH_SKIP_TRAIN=1; this project's sphere kernels only, split by grid size; "
                    "tools/summarize_sphere_insts.py")
    with open(out_path, "w") as fh:
        json.dump(out, fh, indent=1)
    for k, v in out.items():
        if isinstance(v, dict) and "per_wave" in v:
            print(k, v["launches_seen"], v["per_wave"])


if __name__ == "__main__":
    main()
