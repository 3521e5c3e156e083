"""Plays sequences of tests/session_cases.py on the GPU by hand, one step per line with its verdict, and stops at the first mismatch:
the tool for reducing a failure of tests/test_session_gpu.py (find the shortest failing prefix with LAST_STEP, then drop steps in a
copy of the sequence under session_cases.REGRESSIONS).  One pass; nothing is tried again.
usage: python tests/session_replay.py [--layout LAYOUT] SCENE SEED [PART] [LAST_STEP]
SEED: a circuit or walk seed of the scene (the wide seeds, which also draw window and variance steps, and the edit seeds, which also
draw lights, materials, ids, refused_edit, matte_groups and mattes steps, and the post seeds, which also draw clamp, motion_blur and dof
steps and compare the scene's temporal clamp after every step, included: session_cases.SCENES), or the name of a regression; PART: one
sequence of the seed (default: all of them).  LAYOUT: a key of session_cases.LAYOUTS -- the scene is created under its RT_* variables
and every frame that settles is rendered three times, as tests/test_session_gpu.py::test_sequence_under_layout does; what the settled
frames reported of their ordered rounds is printed per sequence."""
import collections, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: F401  (before the library loads its HIP runtime)
import session_cases as SC

args, layout = sys.argv[1:], None
if "--layout" in args:
    at = args.index("--layout")
    if at + 1 >= len(args) or args[at + 1] not in SC.LAYOUTS:
        sys.exit(f"--layout takes one of {', '.join(SC.LAYOUTS)}")
    layout = args[at + 1]
    del args[at:at + 2]
if len(args) < 2:
    sys.exit(__doc__)
name = args[0]
seed = args[1] if args[1] in SC.REGRESSIONS else int(args[1])
count = 1 if seed in SC.REGRESSIONS else len(SC.sequences(name, seed))
parts = [int(args[2])] if len(args) > 2 else list(range(count))
last = int(args[3]) if len(args) > 3 else None


def report(i, step, verdict):
    kind, arg = step
    print(f"  step {i:2d}  {kind}{'' if arg is None else f'({arg})'}: {verdict}", flush=True)


for part in parts:
    print(f"{name} seed {seed} part {part}{f' under the layout {layout}' if layout else ''}, from {SC.part_of(name, seed, part)['start']}", flush=True)
    tally = collections.Counter()
    try:
        SC.play(name, seed, part, last, report, layout=layout, tally=tally)
    except AssertionError as e:
        print(e)
        sys.exit(1)
    if layout:
        print(f"  settled frames (layout, class, trace rounds, placement): {dict(tally)}", flush=True)
print("every step matched")
