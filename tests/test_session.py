"""The session sequences without a GPU (tests/session_cases.py; tests/test_session_gpu.py plays them on the device): generation is
deterministic, every circuit holds every ordered pair of kinds exactly once and cutting loses none, camera and shape steps change the
state; on the oracles alone the visited states are not vacuous (hit shares, changed shares), the caps hold (refusals, accepting
temporal steps, a temporal step on an older frame and a motion step with camera and shape both changed in every circuit), and the
model, driven through the chains of motion_cases.py and temporal_cases.py, gives exactly their states, references and histories."""
import collections

import numpy as np
import pytest

import geometry_cases as GC
import motion_cases as MC
import motion_oracle as MO
import session_cases as SC
import temporal_cases as TC
import temporal_oracle as TO

F32 = np.float32


def circuits():
    return [(name, seed) for name, spec in SC.SCENES.items() for seed in spec["circuits"]]


def every_sequence():
    return [(name, seed, part, SC.part_of(name, seed, part)) for name, seed, part in SC.all_parts()]


# ---- generation -----------------------------------------------------------------------------------------------------------------------
def test_generation_is_deterministic():
    first = {(n, s, p): q for n, s, p, q in every_sequence()}
    SC._sequences.clear()
    again = {(n, s, p): q for n, s, p, q in every_sequence()}
    assert first == again and len(first) == len(SC.all_parts())
    assert dict(sequences=len(first), steps=sum(len(q["steps"]) for q in first.values())) == SC.COUNTS, "the draw changed: measure again"


@pytest.mark.parametrize("name, seed", circuits())
def test_a_circuit_holds_every_ordered_pair_once_and_cutting_loses_none(name, seed):
    parts = SC.sequences(name, seed)
    kinds, end = [], ("home", "home")
    for i, q in enumerate(parts):
        ks = [k for k, _ in q["steps"]]
        assert 2 <= len(ks) <= SC.SCENES[name]["cut"] <= SC.CUT and q["start"] == end
        if i:
            assert ks[0] == kinds[-1], "a sequence does not start with the kind the one before ended in"
            ks = ks[1:]
        kinds += ks
        s = SC.Lite(*q["start"])
        for step in q["steps"]:
            s.advance(step)
        end = (s.pose, s.shape)
    assert len(kinds) == SC.K * SC.K + 1 and kinds[0] == kinds[-1]
    pairs = collections.Counter(zip(kinds, kinds[1:]))
    assert len(pairs) == SC.K * SC.K and set(pairs.values()) == {1} and set(k for k, _ in pairs) == set(SC.KINDS)
    within = collections.Counter(p for q in parts for p in zip([k for k, _ in q["steps"]], [k for k, _ in q["steps"]][1:]))
    assert within == pairs, "a pair is adjacent in the circuit but in none of its sequences"


def test_camera_and_shape_steps_change_the_state_and_refusals_stay_rare():
    for name, seed, part, q in every_sequence():
        s, refused = SC.Lite(*q["start"]), 0
        for kind, arg in q["steps"]:
            if kind in ("camera", "refused_camera"):
                assert arg in SC.POSES and arg != s.pose, (name, seed, part, kind, arg)
            if kind == "shape":
                assert arg in SC.SCENES[name]["shapes"] and arg != s.shape, (name, seed, part, kind, arg)
            if kind == "refused_update":
                assert arg[0] in SC.UPDATE_REFUSALS and arg[1] != s.shape
            refused += bool(s.refuses((kind, arg)))
            s.advance((kind, arg))
        assert refused * 5 <= len(q["steps"]), f"{name} seed {seed} part {part}: {refused} of {len(q['steps'])} steps are refusals"
    for name, spec in SC.SCENES.items():
        for seed in spec["walks"]:
            assert [len(q["steps"]) for q in SC.sequences(name, seed)] == [SC.WALK]


# ---- the visited states and the caps, on the oracles alone -------------------------------------------------------------------------------
_played = {}


def played(name):
    """The model alone over every sequence of the scene: {(seed, part): notes}, the visited states in order of first visit, and the
    (state, next state) pairs of its camera and shape steps."""
    if name not in _played:
        w = SC.world(name)
        notes, states, moves = {}, [], set()
        for n, seed, part, q in every_sequence():
            if n != name:
                continue
            s = SC.Session(w, q["start"])
            states.append(s.here())
            for step in q["steps"]:
                before = s.here()
                s.apply(step)
                if s.here() != before:
                    moves.add((before, s.here()))
                    states.append(s.here())
            notes[seed, part] = s.notes
        _played[name] = (notes, list(dict.fromkeys(states)), sorted(moves))
    return _played[name]


@pytest.mark.parametrize("name", list(SC.SCENES))
def test_visited_states_hit_and_consecutive_states_differ(name):
    w = SC.world(name)
    _, states, moves = played(name)
    hits = []
    for st in states:
        hits.append(float((w.trace(*st)[1] != SC.NONE).mean()))
        assert hits[-1] >= MC.MIN_HIT, f"{name}/{st}: only {hits[-1]:.3f} of the centre rays hit"
    changed = []
    for a, b in moves:
        share = GC.changed_share(w.planes(*a), w.planes(*b))
        if a[0] == b[0] and {a[1], b[1]} <= {"home", "reindex"}:  # the same triangles under other indices (geometry_cases.py: the
            planes_moved = not np.array_equal(w.state(*a).box_min, w.state(*b).box_min)  # planes moved with V, or the frame is the same)
            assert planes_moved or share == 0.0, f"{name}: {a} -> {b}: same planes but another frame"
            continue
        changed.append(share)
        assert share >= GC.MIN_CHANGED, f"{name}: {a} -> {b}: the oracle's planes change in {share:.4f} of the pixels only"
    print(f"{name}: {len(states)} states visited, hit share {min(hits):.3f}..{max(hits):.3f}; {len(moves)} distinct moves, changed share "
          f"{min(changed):.3f}..{max(changed):.3f}")
    assert len(states) >= 12 and states == SC.visited(name)
    assert {p for p, _ in states} == set(SC.POSES) and {n for _, n in states} == set(SC.SCENES[name]["shapes"]), "a pose or shape is never visited"


def test_temporal_and_motion_steps_are_not_vacuous():
    accepting = total = 0
    for name, spec in SC.SCENES.items():
        notes, _, _ = played(name)
        for seed in spec["circuits"]:
            mine = [n for (s, _), ns in notes.items() if s == seed for n in ns]
            assert any(k == "temporal" and stale for k, stale, _ in mine), f"{name} seed {seed}: no temporal step on an older frame"
            assert any(k == "motion" and both for k, both, _ in mine), f"{name} seed {seed}: no motion step with camera and shape both changed"
        for ns in notes.values():
            for k, _, share in ns:
                if k == "temporal":
                    total += 1
                    accepting += share >= TC.MIN_ACCEPT
    print(f"{accepting} of {total} temporal steps accept history in at least {TC.MIN_ACCEPT} of the pixels")
    assert total >= 30 and accepting * 3 >= total


# ---- the model against the chains of the motion and temporal tests ---------------------------------------------------------------------------
def same_state(got, want, label, camera=True):
    for k in (("eye", "eye_to_top_left", "left_to_right", "top_to_bottom") if camera else ()) + ("vertex", "tri_index"):
        assert np.asarray(getattr(got, k)).tobytes() == np.asarray(getattr(want, k)).tobytes(), (label, k)
    assert float(got.pixel_size_inv) == float(want.pixel_size_inv), label


def same_flow(got, want, label):
    for k in want:
        assert MO.same_bits(got[k], want[k]).all(), (label, k)


def test_the_model_gives_the_states_and_references_of_the_motion_chains():
    w = SC.world("mirror_hall")
    sc = w.base
    s = SC.Session(w)
    s.apply(("mark", None))
    for (pose, mark), (_, cur, ref, _, _) in zip(MC.CAMERA_SEQUENCE, MC.camera_steps(sc)):
        if mark:
            s.apply(("mark", None))
        s.apply(("camera", pose))
        s.apply(("motion", None))
        same_state(w.state(*s.here()), cur, f"camera/{pose}: current")
        same_state(w.state(*s.mark), ref, f"camera/{pose}: reference")
        same_flow(w.flow(s.here(), s.mark), MO.motion(cur, ref), f"camera/{pose}")
    s = SC.Session(w)
    s.apply(("mark", None))
    for (name, mark), (_, _, cur, ref, _, _) in zip(MC.GEOMETRY_SEQUENCE, MC.geometry_steps(sc)):
        if mark:
            s.apply(("mark", None))
        s.apply(("shape", name))
        s.apply(("motion", None))
        same_state(w.state(*s.here()), cur, f"geometry/{name}: current")
        same_state(w.state(*s.mark), ref, f"geometry/{name}: reference")
        assert np.array_equal(w.state(*s.here()).grid_list, cur.grid_list), name
        same_flow(w.flow(s.here(), s.mark), MO.motion(cur, ref), f"geometry/{name}")
    assert len(s.notes) == len(MC.GEOMETRY_SEQUENCE)


def test_the_model_gives_the_histories_of_the_temporal_camera_chain():
    w = SC.world("mirror_hall")
    chain = TC.camera_chain(w.base)
    flows = TC.chain_flows([(cur, ref) for _, cur, ref in chain])
    s = SC.Session(w)
    hist = TO.empty_history(w.height, w.width)
    for i, ((pose, cur, ref), flow) in enumerate(zip(chain, flows)):
        if i:
            s.apply(("camera", pose))
        s.apply(("frame", None))
        s.apply(("temporal", (False, 32)))
        colour = np.stack(w.planes(pose, "home"), -1).astype(F32) / F32(65535.0)
        want = TO.accumulate(colour, flow["motion"], flow["prev_t"], flow["triangle"], hist)
        hist = TO.next_history(want, flow["t"], flow["triangle"])
        for k in hist:
            assert TO.same_bits(s.history[k], hist[k]).all(), (pose, k)
        assert s.mark == s.here()
    assert (hist["count"] > 1.0).any()
    s.apply(("reset_temporal", None))
    assert s.history is None
