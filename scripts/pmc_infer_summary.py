"""Reduce a `rocprofv3 --pmc ... --kernel-trace --output-format csv` counter file to one line per kernel (all dispatches summed):
MfmaUtil = SQ_VALU_MFMA_BUSY_CYCLES / (GRBM_GUI_ACTIVE / 8 XCDs x 1024 SIMDs), SQ_WAIT_ANY and SQ_WAIT_INST_ANY as shares of SQ_WAVE_CYCLES,
SQ_LDS_BANK_CONFLICT summed.  Usage: python scripts/pmc_infer_summary.py <k_counter_collection.csv> [kernel-name substring ...]"""
import collections
import csv
import sys


def main(path, keys):
    agg = collections.defaultdict(lambda: collections.defaultdict(float))
    disp = collections.defaultdict(set)
    for r in csv.DictReader(open(path)):
        k = r["Kernel_Name"].replace("void (anonymous namespace)::", "").replace("(anonymous namespace)::", "").split("(")[0]
        if keys and not any(s in k for s in keys):
            continue
        agg[k][r["Counter_Name"]] += float(r["Counter_Value"])
        disp[k].add(r["Dispatch_Id"])
    print("%-40s %5s %9s %9s %10s %9s" % ("kernel", "disp", "MfmaUtil", "wait_any", "wait_inst", "lds_conf"))
    for k, v in sorted(agg.items()):
        u = v["SQ_VALU_MFMA_BUSY_CYCLES"] / (v["GRBM_GUI_ACTIVE"] / 8 * 1024)
        print("%-40s %5d %9.3f %9.3f %10.3f %9.0f" % (k[:40], len(disp[k]), u, v["SQ_WAIT_ANY"] / v["SQ_WAVE_CYCLES"],
                                                  v["SQ_WAIT_INST_ANY"] / v["SQ_WAVE_CYCLES"], v["SQ_LDS_BANK_CONFLICT"]))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])
