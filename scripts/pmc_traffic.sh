# usage: [PMC_PASSES="fetch write rdreq"] bash scripts/pmc_traffic.sh <tag> [workload] -- memory traffic of every kernel: FETCH_SIZE, WRITE_SIZE and
# the fabric read requests (TCC_EA0_RDREQ*, by size) in SEPARATE rocprofv3 --pmc passes (TCC slots), no tracing domains mixed in; writes
# traffic.json into the run's output directory ($out below).  PMC_PASSES picks the passes to run (default: all three).  The library under test is the one
# opencl_render_amd loads (RT_HIP_LIB selects a variant).
set -e
tag=$1; wl=${2:-lambert_1m}
passes=${PMC_PASSES:-fetch write rdreq}
export TMPDIR=/tmp
out=gpurun_out/traffic_$tag
mkdir -p $out
run() { name=$1; shift; timeout -k 10 300 rocprofv3 --pmc "$@" --output-format csv -d $out/$name -- python3 bench.py --workload $wl --steps 4 --warmup 1 --no-cpu-baseline > $out/$name.log 2>&1; }
for p in $passes; do
    case $p in
        fetch) run fetch FETCH_SIZE ;;
        write) run write WRITE_SIZE ;;
        rdreq) run rdreq TCC_EA0_RDREQ_sum TCC_EA0_RDREQ_32B_sum TCC_EA0_RDREQ_64B_sum TCC_EA0_RDREQ_128B_sum ;;
        *) echo "pmc_traffic.sh: unknown pass $p" >&2; exit 2 ;;
    esac
done
python3 - $out $wl <<'PY'
import csv, glob, json, sys, collections
root, wl = sys.argv[1], sys.argv[2]
tot = collections.defaultdict(lambda: collections.defaultdict(float)); calls = collections.defaultdict(collections.Counter)
for f in glob.glob(root + "/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        k = r["Kernel_Name"].split("(")[0].replace("void ", "")
        if not (k.startswith("wf_") or k.startswith("rt_")): continue
        tot[k][r["Counter_Name"]] += float(r["Counter_Value"])
        calls[r["Counter_Name"]][k] += 1
# a frame = one wf_primary_kernel dispatch; every pass runs the same frames, so any counter's dispatch count will do
frames_of = {c: (n.get("wf_primary_kernel", 0) or 1) for c, n in calls.items()}
frames = max(frames_of.values()) if frames_of else 1
res = {"workload": wl, "frames": frames, "note": "counters summed over all dispatches of the run, divided by the run's frames (wf_primary_kernel dispatches); "
       "gfx950: FETCH_SIZE (KB) tallies 128-B fabric reads at 64 B, so read bytes = 2*FETCH_SIZE*1024 (MI355X_MICROARCH.md, HBM); "
       "read_requests = TCC_EA0_RDREQ_sum, with its 32 / 64 / 128-byte parts", "per_frame": {}}
for k, c in tot.items():
    row = {}
    def per_frame(name): return c[name] / frames_of[name]
    if "FETCH_SIZE" in c: row["read_bytes"] = 2.0 * per_frame("FETCH_SIZE") * 1024
    if "WRITE_SIZE" in c: row["write_bytes"] = per_frame("WRITE_SIZE") * 1024
    if "read_bytes" in row and "write_bytes" in row: row["hbm_bytes"] = row["read_bytes"] + row["write_bytes"]
    if "TCC_EA0_RDREQ_sum" in c:
        row["read_requests"] = per_frame("TCC_EA0_RDREQ_sum")
        for size in ("32B", "64B", "128B"):
            if f"TCC_EA0_RDREQ_{size}_sum" in c: row[f"read_requests_{size}"] = per_frame(f"TCC_EA0_RDREQ_{size}_sum")
    any_counter = next(iter(c))
    row["dispatches_per_frame"] = calls[any_counter][k] / frames_of[any_counter]
    res["per_frame"][k] = row
json.dump(res, open(root + "/traffic.json", "w"), indent=1)
for k, v in sorted(res["per_frame"].items()):
    print(f'{k:40s} ' + "  ".join(f"{n} {x:.4g}" for n, x in v.items()))
PY
