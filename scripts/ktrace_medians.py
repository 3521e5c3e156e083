"""Per-launch medians of a kernel trace: python scripts/ktrace_medians.py <trace directory> [more directories ...]

Reads the kernel_trace.csv that scripts/ktrace.sh left in each directory, cuts the run into frames (a frame starts at a wf_primary launch),
keeps the frames whose launch sequence is the run's most common one (the planned frames: a watched frame launches other kernels) and
prints, per launch of that sequence, the median start offset in the frame and the median, minimum and maximum duration over those frames
in microseconds, and the duration figures for the time from the frame's first start to its last end.  With several directories the launches
are printed side by side, one column group per directory (they must share the sequence)."""
import collections
import csv
import glob
import statistics
import sys


def frames_of(directory):
    f = glob.glob(directory + "/**/*kernel_trace.csv", recursive=True)[0]
    rows = [r for r in csv.DictReader(open(f)) if r["Kernel_Name"].startswith(("void wf_", "wf_", "rt_", "void rt_"))]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    frames, cur = [], None
    for r in rows:
        name = r["Kernel_Name"].split("(")[0].replace("void ", "")
        if "wf_primary" in name:
            cur = []
            frames.append(cur)
        if cur is not None:
            cur.append((name, int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    common = collections.Counter(tuple(n for n, _, _ in fr) for fr in frames).most_common(1)[0][0]
    return common, [fr for fr in frames if tuple(n for n, _, _ in fr) == common]


def stats(values, starts=None):
    at = f"{statistics.median(starts):9.1f}" if starts is not None else " " * 9
    return f"{at} {statistics.median(values):9.1f} {min(values):9.1f} {max(values):9.1f}"


def main():
    runs = [frames_of(d) for d in sys.argv[1:]]
    seq = runs[0][0]
    for d, (s, frames) in zip(sys.argv[1:], runs):
        assert s == seq, f"{d}: another launch sequence"
        print(f"# {d}: {len(frames)} frames with the common launch sequence")
    print("# per launch: median start offset, then duration median min max (us)" + " |" * (len(runs) - 1))
    for i, name in enumerate(seq):
        print(f"{i:2d} {name:44s} " + " | ".join(stats([(fr[i][2] - fr[i][1]) / 1e3 for fr in frames], [(fr[i][1] - fr[0][1]) / 1e3 for fr in frames]) for _, frames in runs))
    print(f"   {'first start to last end':44s} " + " | ".join(stats([(max(e for _, _, e in fr) - fr[0][1]) / 1e3 for fr in frames]) for _, frames in runs))


if __name__ == "__main__":
    main()
