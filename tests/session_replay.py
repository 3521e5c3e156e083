"""Plays sequences of tests/session_cases.py on the GPU by hand, one step per line with its verdict, and stops at the first mismatch:
the tool for reducing a failure of tests/test_session_gpu.py (find the shortest failing prefix with LAST_STEP, then drop steps in a
copy of the sequence under session_cases.REGRESSIONS).  One pass; nothing is tried again.
usage: python tests/session_replay.py SCENE SEED [PART] [LAST_STEP]
SEED: a circuit or walk seed of the scene (the wide seeds, which also draw window and variance steps, and the edit seeds, which also
draw lights, materials, ids, refused_edit, matte_groups and mattes steps, and the post seeds, which also draw clamp, motion_blur and dof
steps and compare the scene's temporal clamp after every step, included: session_cases.SCENES), or the name of a regression; PART: one
sequence of the seed (default: all of them)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: F401  (before the library loads its HIP runtime)
import session_cases as SC

if len(sys.argv) < 3:
    sys.exit(__doc__)
name = sys.argv[1]
seed = sys.argv[2] if sys.argv[2] in SC.REGRESSIONS else int(sys.argv[2])
count = 1 if seed in SC.REGRESSIONS else len(SC.sequences(name, seed))
parts = [int(sys.argv[3])] if len(sys.argv) > 3 else list(range(count))
last = int(sys.argv[4]) if len(sys.argv) > 4 else None


def report(i, step, verdict):
    kind, arg = step
    print(f"  step {i:2d}  {kind}{'' if arg is None else f'({arg})'}: {verdict}", flush=True)


for part in parts:
    print(f"{name} seed {seed} part {part}, from {SC.part_of(name, seed, part)['start']}", flush=True)
    try:
        SC.play(name, seed, part, last, report)
    except AssertionError as e:
        print(e)
        sys.exit(1)
print("every step matched")
