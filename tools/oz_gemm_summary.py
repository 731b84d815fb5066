"""k_oz_gemm's launches from rocprofv3 output directories (dev tool, see tools/oz_gemm_profile.sh).
trace: launches and time per launch kind (by grid size: at n = 16384 the Schur complement S has
2424832 threads, T and X21 4194304, the LAUUM 8847360).  pmc: the counters of every launch of one
evaluation, matched across passes by their order; clock = GRBM_GUI_ACTIVE / 8 / time, MFMA busy
= SQ_VALU_MFMA_BUSY_CYCLES / (clock cycles x 1024 SIMDs), as tools/pmc_phases.py; FETCH_SIZE is
in KiB and reports half the bytes of wide streaming reads on gfx950.
usage: oz_gemm_summary.py trace DIR OUT.json   |   oz_gemm_summary.py pmc DIR [DIR ...] OUT.json"""
import csv
import glob
import json
import os
import sys

mode, dirs, out = sys.argv[1], sys.argv[2:-1], sys.argv[-1]


def grid(r):
    for k in ("Grid_Size_X", "Grid_Size", "Workgroup_Size_X"):
        if k in r:
            return int(float(r[k]))
    return -1


if mode == "trace":
    rows = []
    for f in glob.glob(os.path.join(dirs[0], "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "k_oz_gemm" in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), grid(r)))
    rows.sort()
    kinds = {}
    for _, ns, g in rows:
        e = kinds.setdefault(g, {"launches": 0, "ns": 0, "min_ns": 1 << 62, "max_ns": 0})
        e["launches"] += 1
        e["ns"] += ns
        e["min_ns"] = min(e["min_ns"], ns)
        e["max_ns"] = max(e["max_ns"], ns)
    rec = {"launches": len(rows), "total_ms": sum(r[1] for r in rows) / 1e6,
           "by_grid": {str(g): dict(e, mean_ms=e["ns"] / e["launches"] / 1e6) for g, e in sorted(kinds.items())},
           "sequence_tail": [(g, ns / 1e6) for _, ns, g in rows[-20:]]}
else:
    disp = {}
    for d in dirs:
        for f in glob.glob(os.path.join(d, "**", "*counter_collection*.csv"), recursive=True):
            seq = {}
            for r in csv.DictReader(open(f)):
                if "k_oz_gemm" not in r["Kernel_Name"]:
                    continue
                k = int(r["Dispatch_Id"])
                e = seq.setdefault(k, {"grid": grid(r)})
                if "End_Timestamp" in r:
                    e["ns"] = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
                e[r["Counter_Name"]] = e.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
            for i, k in enumerate(sorted(seq)):   # launches matched across passes by their order
                disp.setdefault(i, {}).update(seq[k])
    ls = [disp[i] for i in sorted(disp)]
    for e in ls:
        if "GRBM_GUI_ACTIVE" in e and e.get("ns"):
            e["clock_ghz"] = e["GRBM_GUI_ACTIVE"] / 8 / e["ns"]
            if "SQ_VALU_MFMA_BUSY_CYCLES" in e:
                e["mfma_busy"] = e["SQ_VALU_MFMA_BUSY_CYCLES"] / (e["GRBM_GUI_ACTIVE"] / 8 * 1024)
        if "TCC_HIT_sum" in e:
            e["l2_hit"] = e["TCC_HIT_sum"] / max(e["TCC_HIT_sum"] + e.get("TCC_MISS_sum", 0.0), 1.0)
    rec = {"launches": ls}
json.dump(rec, open(out, "w"), indent=1)
print(json.dumps(rec)[:3000])
