"""kernel_trace.csv of rocprofv3 -> the ordered list of kernel names (by start time) and the call count per kernel."""
import csv, glob, sys
src = glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)
assert len(src) == 1, src
rows = list(csv.DictReader(open(src[0])))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
names = [r["Kernel_Name"] for r in rows]
table = sorted(set(names))
with open(sys.argv[2], "w") as f:
    f.write(f"# {len(names)} launches of {len(table)} kernels\n# calls  id  kernel\n")
    for i, n in enumerate(table):
        f.write(f"{names.count(n):6d}  k{i:<3d} {n}\n")
    f.write("# launch order (ids above), 16 per line\n")
    ids = [f"k{table.index(n)}" for n in names]
    for i in range(0, len(ids), 16):
        f.write(" ".join(ids[i: i + 16]) + "\n")
print(sys.argv[2], len(names), "launches,", len(table), "kernels")
