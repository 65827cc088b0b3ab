"""Reads a rocprofv3 kernel trace of bench.py (..._kernel_trace.csv) and prints the kernels of every stream around the start
of one step's encoder backward, one line each, indented by stream: what runs beside the block-4 convolutions.  Times in
microseconds from the start of freq_mean_bwd_kernel; side-stream kernels shorter than 12 us are left out.
Usage: python tools/stream_timeline.py <kernel_trace.csv> [step index, default -3] [span in us, default 2400]"""
import csv
import sys

rows = sorted(csv.DictReader(open(sys.argv[1])), key=lambda r: int(r["Start_Timestamp"]))
which = int(sys.argv[2]) if len(sys.argv) > 2 else -3
span = float(sys.argv[3]) if len(sys.argv) > 3 else 2400


def nm(r):
    k = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").replace("acvae::", "")
    return k.split("(")[0][:34]


i0 = [i for i, r in enumerate(rows) if "freq_mean_bwd" in r["Kernel_Name"]][which]
t0 = int(rows[i0]["Start_Timestamp"])
main = rows[i0]["Stream_Id"]
for r in rows[max(0, i0 - 60):]:
    s, e = (int(r["Start_Timestamp"]) - t0) / 1e3, (int(r["End_Timestamp"]) - t0) / 1e3
    if s > span:
        break
    if e < -1200 or (e - s < 12 and r["Stream_Id"] != main):
        continue
    sid = int(r["Stream_Id"])
    print(f"{'      ' * min(sid, 3)}s{sid} {s:8.1f} -> {e:8.1f} ({e - s:7.1f}) {nm(r)}")
