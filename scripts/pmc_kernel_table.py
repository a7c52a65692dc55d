"""Reduce the counter_collection.csv files of `rocprofv3 --pmc FETCH_SIZE` and `--pmc WRITE_SIZE` runs of one program (one counter per
run: gfx950 refuses the two in one pass) to one line per (kernel, grid size): dispatches, mean duration, mean FETCH_SIZE / WRITE_SIZE per
dispatch in MB (rocprofv3 reports KiB; FETCH_SIZE reports 0.5 of a stream read with 16-byte lanes, bench.py roofline.traffic_note).
usage: pmc_kernel_table.py DIR [DIR ...] -> CSV on stdout (kernels with fewer than MIN_CALLS = 20 dispatches are left out)"""
import collections, csv, glob, os, sys

acc = collections.defaultdict(lambda: {"n": collections.Counter(), "v": collections.Counter(), "us": 0.0})
files = [f for d in sys.argv[1:] for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)]
for f in files:
    for r in csv.DictReader(open(f)):
        name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("pa::", "").replace("void ", "").split("(")[0][:72]
        a = acc[(name, int(r["Grid_Size"]))]
        a["n"][r["Counter_Name"]] += 1
        a["v"][r["Counter_Name"]] += float(r["Counter_Value"])
        if r["Counter_Name"] == "FETCH_SIZE":
            a["us"] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3
min_calls = int(os.environ.get("MIN_CALLS", "20"))
print("kernel,grid,dispatches,avg_us_under_pmc,fetch_MB,write_MB")
rows = []
for k, a in acc.items():
    n = a["n"]["FETCH_SIZE"]
    if n < min_calls:
        continue
    mb = lambda c: a["v"][c] / max(a["n"][c], 1) * 1024 / 1e6  # noqa: E731
    rows.append((a["us"], f'"{k[0]}",{k[1]},{n},{a["us"] / n:.1f},{mb("FETCH_SIZE"):.2f},{mb("WRITE_SIZE"):.2f}'))
for _, line in sorted(rows, reverse=True):
    print(line)
