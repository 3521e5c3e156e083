"""Resident scenes under sequences of operations: a model of the scene's state, the operations with their effect on the model and their
check, and the seeded sequences (tests/test_session.py shows on the oracles alone that they are not vacuous and that the model is right,
tests/test_session_gpu.py plays them on the device, tests/session_replay.py plays one by hand).

State.  The model (Session) holds the pose (camera_cases.POSES + "shifted") and the shape (geometry_cases.SEQUENCE, deformations of the
BASE scene), the pass mask, the pipeline, the last rendered frame (its planes and the pose, shape and mask it was rendered under), the
motion reference (pose and shape at the mark, or none), the temporal history (temporal_oracle's arrays; None = reset or never made),
whether an update has succeeded (the scene retains an index array from then on) and the pose ResidentScene.scene describes (the one of
creation or of the last update: a camera move does not touch that copy); for the wide seeds (KINDS_WIDE) also the sample window the
next frame renders and the one the last frame rendered, and the live moments of the history (None: stale or absent).  The 5 x 7 Scenes of a base scene (fewer where a scene's
shapes are narrowed) are cached in a World with the oracle's grid, camera lists, planes, centre-ray walks and flows.

Checks.  Frames equal oracle_render as integers -- under a window, oracle_render_window of the model's window, onto the model's planes
where the frame continues from the tile buffer (accumulate, first > 0); the scene's window equals the model's after every step; lists and device arrays equal the oracle's after every move and update; motion equals
motion_oracle against the model's mark; temporal equals temporal_oracle.accumulate over the model's LAST RENDERED planes, the flow of the
CURRENT state against the model's mark, and the model's history; refusals return their code and text and change nothing, which every
later check proves.  temporal_variance equals variance_oracle the same way; a temporal step leaves the moments stale, and the next
variance step starts the history again (count 1, variance 0, the frame's colour).  Passes, denoise, AO and the bake are compared with a twin: a ResidentScene created fresh from the model's Scene
(made once per visited state and closed at once, its products cached for the module); a fresh scene's products are pinned to their
oracles by the feature tests.  The denoiser is also compared with denoise_oracle on the read-backs, and on the small scene AO and the
bake with ao_oracle and bake_oracle, so that twin and subject cannot be wrong alike.  Under a window the twin is set to the frame's
(total, first) for the passes, and the filters' colour input is the model's planes; AO, the bake, ray queries and motion keep twins and
oracles that know nothing of windows.  After every update and in every clone the clip bound equals a fresh scene's and holds every
occupied cell; a clone starts with the default window and leaves its parent's alone.

What the header leaves open is not checked: read_passes, denoise and temporal(denoise=) read buffers that a frame fills under the mask
in effect, so where no frame has been rendered yet, or the last one was rendered under another mask, the operation renders one first
(checked like any frame).  So "A directly followed by B" holds for the kinds of a circuit, while on the device a frame stands between
passes -> read_passes, passes -> denoise, passes -> temporal(denoise=) and between a fresh scene and any of the three.  A stale pose
or shape is defined -- the products are the old frame's -- and is left stale on purpose.

Sequences.  A circuit is an Eulerian circuit of the complete directed graph on the K kinds, loops included: K * K + 1 steps in which
every ordered pair of kinds is adjacent exactly once.  It is cut into sequences of at most CUT steps (fewer on the larger scene, see
SCENES).  A cut is placed as late as the refusal cap allows: a sequence is the longest run whose refusals are at most a fifth of its
steps and after which the rest of the circuit can still be cut that way.  Each sequence starts from a fresh scene, at the pose and
shape the one before ended in, and its first step repeats the previous one's last kind, so no pair is lost at a cut.
Arguments are drawn against a light copy of the state so that camera and shape steps always change something and refusals stay rare;
a draw that misses one of the caps below is drawn again (attempt 0, 1, ...): generation is a pure function of (scene, seed).  The wide
seeds have caps of their own (wide_caps); a window that continues is only ever drawn at first = 0, so no frame continues from a buffer
the header leaves undefined."""
import ctypes

import numpy as np

import ao_oracle
import bake_oracle
import camera_cases as CC
import denoise_oracle as D
import geometry_cases as GC
import motion_cases as MC
import motion_oracle as MO
import oracle_lib as O
import prep_oracle as P
import query_cases as Q
import sample_window_cases as WC
import temporal_oracle as TO
import variance_oracle as VO
from clip_checks import assert_bound
from geometry_checks import assert_device_arrays, prep_of, update_to
from opencl_render_amd import raytrace as R

F32 = np.float32
NONE = 0xFFFFFFFF
KINDS = ("frame", "camera", "shape", "passes", "pipeline", "read_passes", "denoise", "ao", "bake", "intersect", "mark", "motion", "temporal",
         "reset_temporal", "refused_update", "refused_camera", "clone")
K = len(KINDS)
# The alphabet is a property of the seed: the seeds drawn before sample windows and the moments history existed keep KINDS (their
# sequences are what they were), the wide seeds of a scene draw from KINDS_WIDE.
KINDS_WIDE = KINDS + ("window", "variance")
POSES = CC.POSES + ("shifted",)
NEAR = ("home", "pan", "shifted")
SURFACE = R.PASS_NORMAL | R.PASS_ALBEDO
MASKS = (SURFACE, 31, SURFACE | R.PASS_ALPHA, SURFACE, 30, 31, 0, R.PASS_NORMAL, 7)  # mostly with both surface passes: the denoiser runs
DENOISE_VARIANTS = ({}, dict(iterations=3, colour_inv_sigma2=0.5))
TEMPORAL_DENOISE = dict(iterations=2, colour_inv_sigma2=0.5)
MAX_HISTORY = (1, 4, 32)
UPDATE_REFUSALS = ("index", "negative", "smaller_v", "host_pointer", "list_limit")
CUT, WALK = 40, 60
MAX_REFUSED = 0.2  # of any sequence's steps
MIN_WARM = 0.35  # of a seed's temporal steps follow another one of their sequence, with no reset and no update between
# Scenes, with their circuit and walk seeds and the shapes drawn for them.  axis_near_axis_mixed loses "translate": from orbit90 the
# translated mesh is hidden, and the oracle's planes of translate, reindex and home are the same there.
# wide_circuits / wide_walks: the seeds that draw from KINDS_WIDE (a circuit of 19 * 19 + 1 = 362 steps).  axis_near_axis_mixed has four
# tiles, so its wide walk exercises the tile groups' copies of the window.  Its path class is the general one (R.path_class), which
# takes no split logic rounds: playing its sequences once more under RT_WF_LOGIC_SPLIT=0 would run the same kernels, and is left out.
# Its walk of 60 steps is cut in two (walk_cut, the second starting with the first's last kind): played whole it took 6.6 s on the device.
# (Seed 106 meets the caps of the draw at its fifth attempt; 104, 105 and 107..109 meet the same caps after 100 to 630.)
SCENES = {"mirror_hall": dict(size=(24, 16), samples=2, circuits=(1, 2), walks=(101, 102), wide_circuits=(4,), wide_walks=(103,),
                              shapes=GC.SEQUENCE, cut=40),
          "axis_near_axis_mixed": dict(size=(136, 132), samples=2, circuits=(3,), walks=(), wide_circuits=(), wide_walks=(106,),
                                       shapes=tuple(n for n in GC.SEQUENCE if n != "translate"), cut=25, shape_steps=2, walk_cut=31)}
# Measured on the oracle by tests/test_session.py, which prints them, over the visited states (hit share of the centre rays; share of the
# oracle's pixels that differ between the two states of a camera or shape step, home <-> reindex excepted as in geometry_cases.py):
# mirror_hall 33 states visited, hit share 0.596..0.987, changed share 0.591..1.000 over 101
# distinct moves; axis_near_axis_mixed 19 states, hit share 0.746..1.000, changed share 0.195..1.000 over 37 moves (all seeds); 21 of 62
# temporal steps of the seeds of COUNTS accept history in at least 0.2 of the pixels.  COUNTS is asserted there, so that a change of the
# draw cannot leave these figures behind.
COUNTS = dict(sequences=34, steps=1019)
# The wide seeds, counted and measured apart (tests/test_session.py prints the figures and asserts the counts): 44 frames (16 under the
# default window, 10 progressive, 7 over-bright, 7 fixed, 4 of a sequence), 6 of them continue from the tile buffer, 4 of those after a
# camera, shape or pipeline step; 4 progressive runs complete; 2 over-bright frames saturate a value that their D = N frame does not;
# of 20 variance steps 8 are warm, 10 start again over stale moments and 1 goes on with live moments.  WINDOW_SHARES: the mean share of
# the plane values in which a continuing frame differs from the same window rendered from zeros (0.811..0.995 over the 6), and in which
# two successive windows of a sequence differ (2 pairs); the test asserts half of each, which leaves room for another draw.
COUNTS_WIDE = dict(sequences=14, steps=493)
WINDOW_SHARES = dict(continuing=0.950, successive=0.987)
WINDOW_SIZES = (2, 3, 4)  # N / S of a drawn window
VARIANCE_FILTER = dict(iterations=2, spatial_below=2.0)
SMALL = "mirror_hall"  # AO and the bake are also compared with their numpy oracles here
# Reduced sequences of mismatches found by the circuits: name -> (scene, (start pose, start shape), steps).  None so far.
REGRESSIONS = {}


def flags(mask):
    return dict(alpha=bool(mask & R.PASS_ALPHA), depth=bool(mask & R.PASS_DEPTH), triangle=bool(mask & R.PASS_TRIANGLE),
                normal=bool(mask & R.PASS_NORMAL), albedo=bool(mask & R.PASS_ALBEDO))


# ---- the oracle's view of a base scene's 5 x 7 states -------------------------------------------------------------------------------
class World:
    def __init__(self, name):
        self.name, self.size = name, SCENES[name]["size"]
        self.base = MC.base_scene(name, self.size)
        self.width, self.height = self.base.width, self.base.height
        self._shape, self._state, self._planes, self._trace, self._flow, self._prep, self._window = {}, {}, {}, {}, {}, {}, {}
        assert self.base.sample_count == SCENES[name]["samples"]

    def shape_scene(self, shape):
        if shape not in self._shape:
            sc = GC.with_arrays(self.base, *GC.arrays(self.base, shape), lists=False)
            sc.box_min, sc.grid_start, sc.grid_list = O.oracle_scene_grid(sc)
            self._shape[shape] = sc
        return self._shape[shape]

    def prep(self, shape):
        """prep_oracle's records and dense view of the shape (seconds on the larger scene's grid, and a circuit updates to the same
        few shapes many times)."""
        if shape not in self._prep:
            self._prep[shape] = prep_of(self.shape_scene(shape))
        return self._prep[shape]

    def warm(self, states):
        """Everything the checks read of the given (pose, shape) states, made now: a test module's fixture calls this once, so that a
        sequence's time is the device's and the comparisons'."""
        for pose, shape in states:
            self.planes(pose, shape)
            self.trace(pose, shape)
            self.prep(shape)

    def state(self, pose, shape):
        """The Scene of (pose, shape) with the oracle's grid and camera lists."""
        if (pose, shape) not in self._state:
            self._state[pose, shape] = CC.posed(self.shape_scene(shape), pose)
        return self._state[pose, shape]

    def planes(self, pose, shape):
        """oracle_render of the state: three [H, W] u16 planes."""
        if (pose, shape) not in self._planes:
            sc = self.state(pose, shape)
            self._planes[pose, shape] = [np.asarray(p).reshape(sc.height, sc.width).copy() for p in O.oracle_render(sc, threads=16)]
        return self._planes[pose, shape]

    def window_planes(self, pose, shape, total, first, divisor, onto=None):
        """oracle_render_window of the state: the frame of the window {total, first, divisor}, from zeros or onto the planes `onto`
        (the tile buffer a continuing frame finds).  Cached: from zeros per state and window, onto planes also per what they hold."""
        sc = self.state(pose, shape)
        if onto is None and (total, first, divisor) == (sc.sample_count, 0, sc.sample_count):
            return self.planes(pose, shape)
        key = (pose, shape, total, first, divisor) + (() if onto is None else tuple(hash(np.asarray(p).tobytes()) for p in onto))
        if key not in self._window:
            self._window[key] = O.oracle_render_window(sc, total, first, divisor, onto=onto, threads=16)
        return self._window[key]

    def trace(self, pose, shape):
        if (pose, shape) not in self._trace:
            self._trace[pose, shape] = MO.trace(self.state(pose, shape))
        return self._trace[pose, shape]

    def flow(self, cur, ref):
        """motion_oracle.motion of state `cur` against the reference state `ref` ((pose, shape) each)."""
        if (cur, ref) not in self._flow:
            self._flow[cur, ref] = MO.project(self.state(*cur), self.state(*ref), self.trace(*cur))
        return self._flow[cur, ref]


_worlds = {}


def world(name):
    if name not in _worlds:
        _worlds[name] = World(name)
    return _worlds[name]


# ---- twins ---------------------------------------------------------------------------------------------------------------------------
_twin, _twin_ao, _twin_bake, _twin_clip, _oracle_ao, _oracle_bake = {}, {}, {}, {}, {}, {}
_bound_held = set()


def twin(w, pose, shape, mask, total=None, first=0):
    """What a scene created fresh from the state returns under `mask` for a frame of sample ids first+1 .. first+S of a sequence of
    `total` (None: S, the default window): {"passes", "denoise" (one per variant, with both surface passes)}.  Passes depend on neither
    the divisor nor on what the frame continued from, so the twin's window is {total, first, S, 0, 0}; its denoised colour is that
    frame's own.  Its AO image, bake and clip bound go to caches of their own (they do not depend on the mask or the window, the bake
    and the bound not on the pose either)."""
    samples = w.base.sample_count
    total = samples if total is None else total
    key = (w.name, pose, shape, mask) + (() if (total, first) == (samples, 0) else (total, first))
    if key not in _twin:
        t = R.ResidentScene(w.state(pose, shape), 0)
        try:
            out = {}
            if mask:
                t.set_passes(**flags(mask))
            if (total, first) != (samples, 0):
                t.set_sample_window(total, first, samples)
            if (w.name, shape) not in _twin_clip:
                _twin_clip[w.name, shape] = t.clip_planes()
            t.render()
            out["passes"] = t.readback_passes()
            if mask & SURFACE == SURFACE:
                out["denoise"] = [t.denoise(**v) for v in DENOISE_VARIANTS]
            plain = (total, first) == (samples, 0)  # (AO and the bake come from twins that never saw a window)
            if plain and (w.name, pose, shape) not in _twin_ao:
                _twin_ao[w.name, pose, shape] = t.ambient_occlusion(rays=4)
            if plain and (w.name, shape) not in _twin_bake:
                _twin_bake[w.name, shape] = t.bake_ambient_occlusion(16, 16, rays=4, dilate=2)
            _twin[key] = out
        finally:
            t.close()
    return _twin[key]


def twin_ao(w, pose, shape):
    if (w.name, pose, shape) not in _twin_ao:
        twin(w, pose, shape, 0)
    return _twin_ao[w.name, pose, shape]


def twin_bake(w, shape):
    if (w.name, shape) not in _twin_bake:
        twin(w, "home", shape, 0)
    return _twin_bake[w.name, shape]


def twin_clip(w, pose, shape):
    """The clip bound of a fresh scene of the shape (made at `pose`, where AO is likely to ask for the same twin)."""
    if (w.name, shape) not in _twin_clip:
        twin(w, pose, shape, 0)
    return _twin_clip[w.name, shape]


def differs(got, want, what):
    """Raises with the array's name and the number of differing values (floats as bits, a NaN on both sides equal)."""
    g, x = np.asarray(got), np.asarray(want)
    assert g.shape == x.shape and g.dtype == x.dtype, f"{what}: got {g.dtype} {g.shape}, want {x.dtype} {x.shape}"
    same = TO.same_bits(g, x) if g.dtype == F32 else g == x
    bad = int(same.size - np.count_nonzero(same))
    assert bad == 0, f"{what} differs in {bad} of {x.size} values"


def refusal(call, text, what):
    """call() must raise RuntimeError with `text` in the library's last error."""
    try:
        call()
    except RuntimeError:
        assert text in R.last_error(), f"{what}: refused with {R.last_error()!r}, expected {text!r}"
        return
    raise AssertionError(f"{what}: the call succeeded, expected a refusal ({text!r})")


# ---- the light state the arguments are drawn against, and every kind's expected refusal ----------------------------------------------------
def window_kind(win, samples):
    """What a window {N, f, D, accumulate, advance} is called here."""
    N, f, D, acc, adv = win
    if win == (samples, 0, samples, 0, 0):
        return "default"
    if acc and adv:
        return "progressive" if D == N else "overbright"
    return "sequence" if adv else "fixed"


class Lite:
    def __init__(self, pose="home", shape="home", samples=2):
        self.pose, self.shape, self.mask, self.pipeline = pose, shape, 0, R.PIPELINE_WAVEFRONT
        self.frame = self.mark = None  # (pose, shape, mask, total, first) / (pose, shape)
        self.updated = False
        # sample windows: the window the next frame renders, the one the last frame rendered (None before the first), and what
        # tests/test_session.py and the caps of the draw ask about every rendered frame (self.frames, one dict per frame)
        self.samples = samples
        self.window_next, self.window_last = (samples, 0, samples, 0, 0), None
        self.frames, self.moved, self.run = [], False, None

    def refuses(self, step):
        kind, arg = step
        if kind == "window":
            return arg is not None and arg[0] == "refused"
        if kind == "variance":
            return arg[0] and self.mask & SURFACE != SURFACE
        if kind == "passes":
            return self.pipeline == R.PIPELINE_MEGAKERNEL and arg != 0
        if kind == "pipeline":
            return arg == R.PIPELINE_MEGAKERNEL and self.mask != 0
        if kind == "denoise":
            return self.mask & SURFACE != SURFACE
        if kind == "motion":
            return self.mark is None
        if kind == "temporal":
            return arg[0] and self.mask & SURFACE != SURFACE
        if kind == "clone":
            return bool(arg)  # the subset's temporal() is refused
        return kind in ("refused_update", "refused_camera")

    def renders(self, uses_passes):
        return self.frame is None or (uses_passes and self.frame[2] != self.mask)

    def advance(self, step):
        """The step's effect on (pose, shape, mask, pipeline, frame, mark, updated); a refused step has none."""
        kind, arg = step
        if self.refuses(step) and kind != "clone":
            return
        if kind == "camera":
            self.pose, self.moved, self.run = arg, True, None
        elif kind == "shape":
            self.shape, self.updated, self.moved, self.run = arg, True, True, None
        elif kind == "passes":
            self.mask = arg
        elif kind == "pipeline":
            self.moved |= arg != self.pipeline
            self.pipeline = arg
        elif kind == "mark":
            self.mark = (self.pose, self.shape)
        elif kind == "window":
            self.window_next, self.run = (arg if arg is not None else (self.samples, 0, self.samples, 0, 0)), None
        if (kind == "frame" or (kind in ("read_passes", "denoise") and self.renders(True))
                or (kind in ("temporal", "variance") and self.renders(arg[0]))):
            self.render_frame()
        if kind in ("temporal", "variance"):
            self.mark = (self.pose, self.shape)

    def render_frame(self):
        """A frame is issued: it renders window_next, which becomes window_last and moves on if it advances.  Notes in self.frames what
        the frame was: its window and the kind of it, whether it continued from the tile buffer and whether a camera, shape or pipeline
        step was made since the frame before, and `complete`: N where this frame ends a progressive run that started at f = 0 and saw
        no camera, shape or window step since (the tile buffer then holds the N-sample frame of the state), else 0."""
        S = self.samples
        N, f, D, acc, adv = win = self.window_next
        kind = window_kind(win, S)
        if kind == "progressive" and f == 0:
            self.run = N
        elif kind != "progressive":
            self.run = None
        complete = N if self.run == N and kind == "progressive" and f == N - S else 0
        self.frames.append(dict(state=(self.pose, self.shape), window=win, kind=kind, continuing=bool(acc and f > 0), moved=self.moved,
                                complete=complete))
        self.frame, self.window_last, self.moved = (self.pose, self.shape, self.mask, N, f), win, False
        if adv:
            self.window_next = (N, (f + S) % N, D, acc, adv)
        if complete:
            self.run = None


def draw(rng, kind, s, may_refuse, tiles, shapes, seen=()):
    """The argument of a step of `kind` in light state `s`; may_refuse: the sequence can still afford a refusal."""
    pick = lambda seq: seq[int(rng.integers(len(seq)))]  # noqa: E731
    dare = may_refuse and rng.random() < 0.3
    if kind == "camera":  # a pose the circuit has not seen yet goes first, so that every circuit visits all five; after that the draw
        new = [p for p in POSES if p not in seen]  # stays among home, pan and shifted, which lie close together, so that history is accepted
        if new:
            return pick(new)
        near = [p for p in NEAR if p != s.pose]
        return pick(near)
    if kind == "shape":
        return pick([n for n in shapes if n != s.shape])
    if kind == "passes":
        if s.pipeline == R.PIPELINE_MEGAKERNEL:
            return pick([m for m in MASKS if m]) if dare else 0
        return pick(MASKS)
    if kind == "pipeline":
        if s.mask:
            return R.PIPELINE_MEGAKERNEL if dare else R.PIPELINE_WAVEFRONT
        if s.pipeline == R.PIPELINE_MEGAKERNEL:
            return R.PIPELINE_WAVEFRONT if rng.random() < 0.8 else R.PIPELINE_MEGAKERNEL
        return R.PIPELINE_MEGAKERNEL if rng.random() < 0.35 else R.PIPELINE_WAVEFRONT
    if kind == "denoise":
        return int(rng.integers(len(DENOISE_VARIANTS)))
    if kind == "intersect":
        return int(rng.integers(1 << 20))
    if kind == "temporal":
        on = rng.random() < 0.5 if s.mask & SURFACE == SURFACE else dare
        return (bool(on), int(pick(MAX_HISTORY)))
    if kind == "refused_update":
        return (pick(UPDATE_REFUSALS), pick([n for n in shapes if n != s.shape]))
    if kind == "refused_camera":
        return pick([p for p in POSES if p != s.pose])
    if kind == "clone":
        return bool(tiles > 1 and dare)
    if kind == "variance":
        on = rng.random() < 0.5 if s.mask & SURFACE == SURFACE else dare
        return (bool(on), int(pick(MAX_HISTORY)))
    if kind == "window":
        S = s.samples
        if dare:  # one of the refusals that apply to a scene of S samples: returns -1 with its text and changes nothing
            _, win, text = pick([r for r in WC.REFUSALS if r[0] == S])
            return ("refused", win, text)
        N = S * int(pick(WINDOW_SIZES))
        r = rng.random()
        if r < 0.08:
            return None  # the default window
        if r < 0.43:  # (a short progressive run is the likeliest to complete before the next move)
            return _progressive(rng, S, N)
        if r < 0.62:
            return (N, 0, S, 0, 1)  # a sequence
        if r < 0.85:
            return (N, 0, S, 1, 1)  # over-bright progressive: every frame at full brightness on top of the frames before
        return (N, int(rng.integers(1, N - S + 1)), int(pick((1, 3, S, N))), 0, 0)  # fixed, off the grid of S where N allows
    return None


def _progressive(rng, S, N):
    """{N, 0, N, 1, 1}; half of them the shortest run, N = 2 S."""
    N = 2 * S if rng.random() < 0.5 else N
    return (N, 0, N, 1, 1)


def eulerian(rng, K=K):
    """K * K + 1 kind indices: a walk that uses every ordered pair of kinds, loops included, exactly once (Hierholzer, the edges of every
    node in a seeded order)."""
    out = [[int(v) for v in rng.permutation(K)] for _ in range(K)]
    stack, path = [int(rng.integers(K))], []
    while stack:
        if out[stack[-1]]:
            stack.append(out[stack[-1]].pop())
        else:
            path.append(stack.pop())
    return path[::-1]


def _piece(rng, kinds, start, tiles, shapes, seen, samples=2):
    """Steps for `kinds` from a fresh scene at `start`, and what the caps ask about them: (steps, refusals after each step, temporal
    steps on an older frame, motion steps with camera and shape both changed, temporal steps, the warm ones among them, each as the
    index of the step; and of the variance steps [(index, warm, stale moments over a live history)])."""
    s, steps, refused, stale, mixed = Lite(*start, samples=samples), [], [], [], []
    seen, hist, temporal, warm = set(seen), False, [], []
    moments, variance = False, []
    for i, k in enumerate(kinds):
        kind = KINDS_WIDE[k]
        step = (kind, draw(rng, kind, s, (sum(refused[-1:]) + 1) <= MAX_REFUSED * (i + 1), tiles, shapes, seen))
        refused.append((refused[-1] if refused else 0) + bool(s.refuses(step)))
        if kind == "temporal" and not s.refuses(step) and not s.renders(step[1][0]) and s.frame[:2] != (s.pose, s.shape):
            stale.append(i)
        if kind == "motion" and s.mark is not None and s.mark[0] != s.pose and s.mark[1] != s.shape:
            mixed.append(i)
        if kind == "temporal" and not s.refuses(step):  # with a history, and reprojected from the same shape: likely to accept some
            temporal.append(i)
            if hist and s.mark[1] == s.shape:
                warm.append(i)
            hist, moments = True, False
        if kind == "variance" and not s.refuses(step):  # warm as a temporal step is: a history, reprojected from the same shape
            variance.append((i, bool(hist and s.mark[1] == s.shape), bool(hist and not moments)))
            hist = moments = True
        if kind == "reset_temporal":
            hist = moments = False
        s.advance(step)
        steps.append(step)
        seen |= {s.pose, s.shape}
    return steps, refused, stale, mixed, temporal, warm, variance


def _attempt(name, seed, attempt):
    """One draw of the seed's sequences, or None where it misses a cap.  A circuit is cut where the refusal cap allows: a piece is the
    longest run of at most the scene's cut whose refusals are at most MAX_REFUSED of its steps, drawn with a generator of its own, and
    the next piece starts with its last kind."""
    spec = SCENES[name]
    key = [sorted(SCENES).index(name), seed, attempt]
    tiles = R.tile_count(*spec["size"])
    walk = seed in spec["walks"] + spec["wide_walks"]
    wide = seed in spec["wide_circuits"] + spec["wide_walks"]
    k = len(kinds_of(name, seed))
    kinds = [int(v) for v in np.random.default_rng(key).integers(k, size=WALK)] if walk else eulerian(np.random.default_rng(key), k)
    limit = spec.get("walk_cut", WALK) if walk else spec["cut"]
    whole = walk and limit == WALK  # (a walk is one sequence, unless the scene cuts its walks as it cuts a circuit)
    budget = [400]  # pieces tried: a draw that needs more is given up

    def rest(at, start, seen):
        """The pieces from step `at` on, or None: the longest piece that fits first, a shorter one where the rest cannot be cut."""
        if at >= len(kinds) - 1:
            return []
        budget[0] -= 1
        if budget[0] < 0:
            return None
        piece = kinds[at:at + limit]
        steps, refused, st, mx, tp, wm, vr = _piece(np.random.default_rng(key + [at]), piece, start, tiles, spec["shapes"], seen,
                                                    spec["samples"])
        for n in range(len(piece), 1, -1):
            if refused[n - 1] > MAX_REFUSED * n or (whole and n < len(piece)):
                continue
            if sum(k == "shape" for k, _ in steps[:n]) > spec.get("shape_steps", n):
                continue  # (an update's check of the device arrays takes over a second on the larger scene's 12.6 million pairs)
            s, now = Lite(*start, samples=spec["samples"]), set(seen)
            for step in steps[:n]:
                s.advance(step)
                now |= {s.pose, s.shape}
            tail = rest(at + n - 1, (s.pose, s.shape), now)
            if tail is not None:
                return [dict(start=start, steps=steps[:n], stale=sum(i < n for i in st), mixed=sum(i < n for i in mx), seen=now,
                             temporal=sum(i < n for i in tp), warm=sum(i < n for i in wm), variance=[v for v in vr if v[0] < n],
                             frames=s.frames)] + tail
        return None

    out = rest(0, ("home", "home"), {"home"})
    if out is None:
        return None
    stale, mixed, seen = sum(q.pop("stale") for q in out), sum(q.pop("mixed") for q in out), set().union(*(q.pop("seen") for q in out))
    variance, frames = [v for q in out for v in q.pop("variance")], [q.pop("frames") for q in out]
    if sum(q.pop("warm") for q in out) < MIN_WARM * sum(q.pop("temporal") for q in out):
        return None  # (too few temporal steps with a history to reproject: the accepting share could not reach a third)
    if wide and not wide_caps(frames, variance, walk):
        return None
    if not walk and not (stale and mixed and seen >= set(POSES) | set(spec["shapes"])):
        return None  # (the camera draw favours the near poses: a circuit still visits every pose and every shape)
    return out


def successive(frames):
    """(i, i + 1) of the frames of one sequence that are successive windows of a sample sequence rendered in the same state."""
    return [(i, i + 1) for i, (a, b) in enumerate(zip(frames, frames[1:])) if a["kind"] == b["kind"] == "sequence"
            and a["state"] == b["state"] and a["window"][0] == b["window"][0] and a["window"][1] != b["window"][1]]


def wide_caps(frames, variance, walk):
    """What a wide seed's draw must hold, from the frames its sequences render (Lite.frames, one list per sequence) and its variance steps [(index, warm,
    stale moments over a live history)].  Every seed: a progressive run completes, and a variance step finds stale moments over a live
    history; a third of the frames under another window than the default, one frame in ten continuing from the tile buffer, half of
    those after a camera, shape or pipeline step made since the frame they continue, and a third of the variance steps warm (a history,
    reprojected from the same shape: the sense of MIN_WARM).  A circuit also: an over-bright frame that continues, and two successive
    frames of a sequence in one state.  tests/test_session.py asserts all of it on the oracle, over the wide seeds together."""
    pairs = [p for part in frames for p in successive(part)]
    frames = [f for part in frames for f in part]
    if not any(f["complete"] for f in frames) or not any(stale for _, _, stale in variance):
        return False
    cont = [f for f in frames if f["continuing"]]
    if not (3 * sum(f["kind"] != "default" for f in frames) >= len(frames) and 10 * len(cont) >= len(frames)
            and 2 * sum(f["moved"] for f in cont) >= len(cont) and 3 * sum(w for _, w, _ in variance) >= len(variance)):
        return False
    return walk or (any(f["kind"] == "overbright" for f in cont) and bool(pairs))


def kinds_of(name, seed):
    """The alphabet of a seed."""
    spec = SCENES[name]
    return KINDS_WIDE if seed in spec["wide_circuits"] + spec["wide_walks"] else KINDS


_sequences = {}


def sequences(name, seed):
    """[{"start": (pose, shape), "steps": [(kind, argument)]}] of a circuit or walk seed of scene `name`."""
    if (name, seed) not in _sequences:
        for attempt in range(2000):
            out = _attempt(name, seed, attempt)
            if out is not None:
                break
        else:
            raise RuntimeError(f"{name} seed {seed}: no draw met the caps")
        _sequences[name, seed] = out
    return _sequences[name, seed]


def seeds_of(name, wide=None):
    """The scene's seeds: all of them, the wide ones (wide=True) or the others (wide=False)."""
    spec = SCENES[name]
    old, new = spec["circuits"] + spec["walks"], spec["wide_circuits"] + spec["wide_walks"]
    return old + new if wide is None else new if wide else old


def all_parts():
    """(scene, seed, part) of every sequence; regressions are (scene, name, 0)."""
    out = [(name, seed, part) for name, spec in SCENES.items() for seed in seeds_of(name) for part in range(len(sequences(name, seed)))]
    return out + [(scene, key, 0) for key, (scene, _, _) in REGRESSIONS.items()]


def visited(name):
    """The (pose, shape) states the scene's sequences pass through, in order of first visit."""
    out = []
    for n, seed, part in all_parts():
        if n == name:
            q = part_of(n, seed, part)
            s = Lite(*q["start"], samples=SCENES[n]["samples"])
            out.append((s.pose, s.shape))
            for step in q["steps"]:
                s.advance(step)
                out.append((s.pose, s.shape))
    return list(dict.fromkeys(out))


def warm_wide(name):
    """The model alone over the scene's wide sequences: every window frame, flow and accumulation their checks read is made now (the
    caches are the World's), as World.warm does for the planes of the visited states."""
    for seed in seeds_of(name, wide=True):
        for q in sequences(name, seed):
            s = Session(world(name), q["start"])
            for step in q["steps"]:
                s.apply(step)


def part_of(name, seed, part):
    if seed in REGRESSIONS:
        scene, start, steps = REGRESSIONS[seed]
        return dict(start=start, steps=list(steps))
    return sequences(name, seed)[part]


# ---- the model, and the device beside it ---------------------------------------------------------------------------------------------
class Session(Lite):
    """The model of one resident scene.  With rs (a ResidentScene created from world.state(*start)) every step is also made on the device
    and checked; without, the model advances alone and notes what tests/test_session.py asserts on (self.notes)."""

    def __init__(self, w, start=("home", "home"), rs=None):
        super().__init__(*start, samples=w.base.sample_count)
        self.w, self.rs = w, rs
        self.described_pose = start[0]
        self.planes = self.history = None
        self.moments = None  # the live moments [H, W, 2] of the history; None: stale (a temporal step wrote none) or absent
        self.notes = []

    def here(self):
        return (self.pose, self.shape)

    def apply(self, step):
        kind, arg = step
        getattr(self, "do_" + kind)(arg) if arg is not None else getattr(self, "do_" + kind)()
        self.advance(step)
        if self.rs:
            self.same_window(f"after {kind}")

    # -- frames
    def do_frame(self):
        """The frame of window_next: the window oracle's, onto the model's planes where the frame continues from the tile buffer."""
        N, f, D, acc, adv = self.window_next
        onto = self.planes if acc and f > 0 else None
        assert onto is not None or not (acc and f > 0), "a frame continues before the sequence's first frame: the header leaves the buffer open"
        want = self.w.window_planes(self.pose, self.shape, N, f, D, onto)
        if self.rs:
            self.rs.render()
            sc = self.w.base
            for ch, g, x in zip("RGB", self.rs.readback(), want):
                differs(np.asarray(g).reshape(sc.height, sc.width), x, f"plane {ch} of the frame at {self.here()} under the window {self.window_next}")
        self.before, self.planes = self.planes, want

    def render_frame(self):
        super().render_frame()
        self.notes.append(("frame", self.frames[-1], (self.before, self.planes)))  # (what the buffer held, what it holds now)

    def need_frame(self, uses_passes):
        if self.renders(uses_passes):
            self.do_frame()
            self.render_frame()

    def same_window(self, what):
        zero = dict(total=0, first=0, divisor=0, accumulate=0, advance=0)
        as_dict = lambda v: dict(zip(("total", "first", "divisor", "accumulate", "advance"), v))  # noqa: E731
        want = {"next": as_dict(self.window_next), "last": zero if self.window_last is None else as_dict(self.window_last)}
        got = self.rs.sample_window()
        assert got == want, f"{what}: the scene's sample window is {got}, the model's {want}"

    def do_window(self, arg=None):
        if not self.rs:
            return
        if self.refuses(("window", arg)):
            _, win, text = arg
            rc = int(R.lib().rtHipSceneSetSampleWindow(self.rs.handle, ctypes.byref(R.SampleWindow(*win))))
            assert rc == -1 and text in R.last_error(), f"refused window {win}: returned {rc} with {R.last_error()!r}, expected -1 with {text!r}"
        elif arg is None:
            self.rs.set_sample_window()
        else:
            self.rs.set_sample_window(*arg)

    # -- state changes
    def do_camera(self, pose):
        sc = self.w.state(pose, self.shape)
        if self.rs:
            self.rs.set_camera(sc.eye, sc.eye_to_top_left, sc.left_to_right, sc.top_to_bottom, sc.pixel_size_inv)
            CC.assert_lists_equal(self.rs, sc, f"lists after the move to {pose}")

    def do_shape(self, name):
        want = self.w.state(self.pose, name)
        if self.rs:
            update_to(self.rs, want)
            CC.assert_lists_equal(self.rs, want, f"lists after the update to {name}")
            assert_device_arrays(self.rs, want, f"device arrays after the update to {name}", self.w.prep(name))
            self.same_bound(self.rs, name, f"the clip bound after the update to {name}")
        self.described_pose = self.pose

    def same_bound(self, rs, shape, what):
        """The kept planes are a fresh scene's, and they hold every corner of every occupied cell."""
        kept = rs.clip_planes()
        differs(kept, twin_clip(self.w, self.pose, shape), what + " (against the twin)")
        # (the corners of a million occupied cells take a second on the larger scene: the same planes over the same block table
        # have the same verdict, and clones of one shape are many)
        key = (self.w.name, shape, kept.tobytes(), hash(rs.scene_view("block_sparse").tobytes()))
        if key not in _bound_held:
            assert_bound(rs, self.w.shape_scene(shape).box_min, what)
            _bound_held.add(key)

    def do_passes(self, mask):
        if not self.rs:
            return
        if self.refuses(("passes", mask)):
            refusal(lambda: self.rs.set_passes(**flags(mask)), "wavefront pipeline", "passes on the megakernel")
        else:
            self.rs.set_passes(**flags(mask))

    def do_pipeline(self, p):
        if not self.rs:
            return
        if self.refuses(("pipeline", p)):
            refusal(lambda: self.rs.set_pipeline(p), "render passes are on", "the megakernel while passes are on")
        else:
            self.rs.set_pipeline(p)

    # -- products of (pose, shape, mask)
    def do_read_passes(self):
        self.need_frame(True)
        if self.rs:
            got, want = self.rs.readback_passes(), twin(self.w, *self.frame)["passes"]
            assert sorted(got) == sorted(want), f"passes {sorted(got)}, the twin's {sorted(want)}"
            for k in want:
                differs(got[k], want[k], f"pass {k} of the frame at {self.frame}")

    def do_denoise(self, variant):
        params = DENOISE_VARIANTS[variant]
        if self.refuses(("denoise", variant)):
            if self.rs:
                refusal(lambda: self.rs.denoise(**params), "normal and the albedo pass", "denoise without both surface passes")
            return
        self.need_frame(True)
        if self.rs:
            got, made = self.rs.denoise(**params), twin(self.w, *self.frame)
            if self.window_last[2:4] == (self.samples, 0):  # the twin's frame is this frame: its divisor is S and neither continued
                want = made["denoise"][variant]
                differs(got["colour"], want["colour"], "denoised colour (against the twin)")
                for ch, g, x in zip("RGB", got["planes"], want["planes"]):
                    differs(g, x, f"denoised plane {ch} (against the twin)")
            # the colour input is the tile buffer, whatever window filled it: the read-backs the oracle is fed are the model's planes
            # and the twin's surface passes
            sc = self.w.base
            planes = [np.asarray(p).reshape(sc.height, sc.width) for p in self.rs.readback()]
            surf = self.rs.readback_passes()
            for ch, g, x in zip("RGB", planes, self.planes):
                differs(g, x, f"plane {ch} of the tile buffer the denoiser read")
            for k in ("normal", "albedo"):
                differs(surf[k], made["passes"][k], f"pass {k} the denoiser read")
            exp = D.denoise(*D.inputs(planes, surf["normal"], surf["albedo"]), **dict(R.DENOISE_DEFAULTS, **params))
            differs(got["colour"], exp, "denoised colour (against the oracle on the read-backs)")
            for ch, g, x in zip("RGB", got["planes"], D.quantise(exp)):
                differs(g, x, f"denoised plane {ch} (against the oracle on the read-backs)")

    def do_ao(self):
        if self.rs:
            got = self.rs.ambient_occlusion(rays=4)
            differs(got, twin_ao(self.w, *self.here()), "AO image (against the twin)")
            if self.w.name == SMALL:
                key = (self.w.name,) + self.here()
                if key not in _oracle_ao:
                    _oracle_ao[key] = ao_oracle.ambient_occlusion(self.w.state(*self.here()), rays=4)
                differs(got, _oracle_ao[key], "AO image (against the oracle)")

    def do_bake(self):
        if self.rs:
            got, want = self.rs.bake_ambient_occlusion(16, 16, rays=4, dilate=2), twin_bake(self.w, self.shape)
            for k in ("ao", "triangle"):
                differs(got[k], want[k], f"bake {k} (against the twin)")
            if self.w.name == SMALL:
                key = (self.w.name, self.shape)
                if key not in _oracle_bake:
                    _oracle_bake[key] = bake_oracle.bake(self.w.state("home", self.shape), 16, 16, rays=4, dilate_passes=2)
                for k in ("ao", "triangle"):
                    differs(got[k], _oracle_bake[key][k], f"bake {k} (against the oracle)")

    def do_intersect(self, seed):
        if self.rs:
            rng = np.random.default_rng(seed)
            o = (rng.normal(size=(256, 3)) * 0.5 + CC.CENTRE).astype(F32)
            d = rng.normal(size=(256, 3)).astype(F32)
            rays = Q._set(o, d, 0.0, np.inf, NONE)
            got = self.rs.intersect(rays["o"], rays["d"], rays["tmin"], rays["tmax"], rays["excluded"])
            bad = Q.mismatches({k: got[k] for k in ("triangle", "t", "ab", "ac")}, Q.oracle_answers(self.w.state(*self.here()), rays))
            assert bad.size == 0, f"ray query answers differ in {bad.size} of 256 rays"

    # -- motion and temporal accumulation
    def same_mark(self, what):
        cam, sc = self.rs.motion_reference_camera(), self.w.state(*self.here())
        for k in ("eye", "eye_to_top_left", "left_to_right", "top_to_bottom"):
            differs(cam[k][:3], np.asarray(getattr(sc, k), F32)[:3], f"{what}: the reference camera's {k}")

    def do_mark(self):
        if self.rs:
            self.rs.mark_motion()
            self.same_mark("mark")

    def do_motion(self):
        if self.mark is None:  # the header: refused with "no motion reference"
            if self.rs:
                refusal(self.rs.motion, "no motion reference", "motion without a mark")
            return
        want = self.w.flow(self.here(), self.mark)
        self.notes.append(("motion", self.mark[0] != self.pose and self.mark[1] != self.shape, MC.shares(want)[0]))
        if self.rs:
            got = self.rs.motion()
            for k in ("motion", "t", "prev_t", "triangle"):
                differs(got[k], want[k], f"motion output {k} at {self.here()} against the mark at {self.mark}")

    def do_temporal(self, arg):
        on, cap = arg
        if self.refuses(("temporal", arg)):
            if self.rs:
                refusal(lambda: self.rs.temporal(denoise=TEMPORAL_DENOISE, max_history=float(cap)), "normal and the albedo pass",
                        "temporal(denoise=) without both surface passes")
            return
        self.need_frame(on)
        flow = self.w.flow(self.here(), self.mark or self.here())  # no mark yet: the call marks the current state first
        colour = np.stack(self.planes, -1).astype(F32) / F32(65535.0)
        hist = self.history if self.history is not None else TO.empty_history(self.w.height, self.w.width)
        acc = TO.accumulate(colour, flow["motion"], flow["prev_t"], flow["triangle"], hist, max_history=float(cap), with_taps=True)
        self.notes.append(("temporal", self.frame[:2] != self.here(), float(acc["used"].mean())))
        if self.rs:
            shown = acc["colour"]
            if on:
                surf = twin(self.w, *self.frame)["passes"]
                shown = D.denoise(acc["colour"], surf["normal"], surf["albedo"], **dict(R.DENOISE_DEFAULTS, **TEMPORAL_DENOISE))
            got = self.rs.temporal(denoise=TEMPORAL_DENOISE if on else None, max_history=float(cap))
            differs(got["count"], acc["count"], "temporal count")
            differs(got["colour"], shown, "temporal colour")
            for ch, g, x in zip("RGB", got["planes"], D.quantise(shown)):
                differs(g, x, f"temporal plane {ch}")
            self.same_mark("temporal (the call owns the mark)")
        self.history = TO.next_history(dict(colour=acc["colour"], count=acc["count"]), flow["t"], flow["triangle"])
        self.moments = None  # the plain call writes none: they are stale from here on

    def do_variance(self, arg):
        """rs.temporal_variance: the accumulation with the luminance moments carried along, over the model's planes, the flow against
        the mark and the model's history; a live history whose moments are stale starts again, as after a reset."""
        on, cap = arg
        if self.refuses(("variance", arg)):
            if self.rs:
                refusal(lambda: self.rs.temporal_variance(filter=VARIANCE_FILTER, max_history=float(cap)), "normal and the albedo pass",
                        "temporal_variance(filter=) without both surface passes")
            return
        self.need_frame(on)
        flow = self.w.flow(self.here(), self.mark or self.here())
        colour = np.stack(self.planes, -1).astype(F32) / F32(65535.0)
        stale = self.history is not None and self.moments is None
        live = self.history is not None and not stale
        hist = dict(self.history, moments=self.moments) if live else VO.empty_history(self.w.height, self.w.width)
        acc = VO.accumulate(colour, flow["motion"], flow["prev_t"], flow["triangle"], hist, max_history=float(cap))
        if not live:  # no history, or one that starts again: the frame itself
            assert (acc["count"] == 1.0).all() and (acc["variance"] == 0.0).all() and TO.same_bits(acc["colour"], colour).all()
        warm = self.history is not None and self.mark is not None and self.mark[1] == self.shape  # (as _piece counts it)
        self.notes.append(("variance", dict(stale=stale, warm=warm, live=live), float((acc["count"] > 1.0).mean())))
        if self.rs:
            shown = dict(colour=acc["colour"], variance=acc["variance"])
            if on:
                surf = twin(self.w, *self.frame)["passes"]
                shown["colour"], shown["variance"] = VO.denoise(acc["colour"], surf["normal"], surf["albedo"], acc["moments"], acc["count"],
                                                                **VARIANCE_FILTER)
            got = self.rs.temporal_variance(filter=VARIANCE_FILTER if on else None, max_history=float(cap))
            differs(got["count"], acc["count"], "temporal_variance count")
            differs(got["colour"], shown["colour"], "temporal_variance colour")
            differs(got["variance"], shown["variance"], "temporal_variance variance")
            for ch, g, x in zip("RGB", got["planes"], D.quantise(shown["colour"])):
                differs(g, x, f"temporal_variance plane {ch}")
            self.same_mark("temporal_variance (the call owns the mark)")
        self.history = TO.next_history(dict(colour=acc["colour"], count=acc["count"]), flow["t"], flow["triangle"])
        self.moments = acc["moments"]

    def do_reset_temporal(self):
        if self.rs:
            self.rs.reset_temporal()
        self.history = self.moments = None

    # -- refusals: one illegal argument each; nothing changes, which every later check proves
    def do_refused_update(self, arg):
        variant, target = arg
        cur, want = self.w.state(*self.here()), self.w.state(self.pose, target)
        if not self.rs:
            assert len(want.grid_list) > 1
            return
        rs, T, V = self.rs, want.triangle_count, want.vertex_count
        if variant == "index":
            bad = want.tri_index.copy()
            bad[T // 2, 1] = V
            rc, code, text = rs.try_set_vertices(want.vertex, bad), -5, P.rejection_text(P.ERR_TRI_INDEX)
        elif variant == "negative":
            bad = want.tri_index.copy()
            bad[0, 0] = -1
            rc, code, text = rs.try_set_vertices(want.vertex, bad), -5, P.rejection_text(P.ERR_TRI_INDEX)
        elif variant == "smaller_v":  # the retained index array against half the vertices; nothing retained before the first update
            rc = rs.try_set_vertices(cur.vertex[: cur.vertex_count // 2])
            code, text = (-5, P.rejection_text(P.ERR_TRI_INDEX)) if self.updated else (-1, "retained")
        elif variant == "host_pointer":
            rc = int(R.lib().rtHipSceneSetGeometry(rs.handle, R.GeometryUpdate(V, R._ptr(want.vertex), None, None, 1)))
            code, text = -1, "not device memory" if self.updated else "retained"
        else:
            R.tune("build_list_limit", len(want.grid_list) - 1)
            try:
                rc, code, text = rs.try_set_vertices(want.vertex, want.tri_index), -3, "limit"
            finally:
                R.tune("build_list_limit", 0xFFFFFFFF)
        assert rc == code and text in R.last_error(), f"refused update ({variant}): returned {rc} with {R.last_error()!r}, expected {code} with {text!r}"

    def do_refused_camera(self, pose):
        sc = self.w.state(pose, self.shape)
        total = int((sc.cam_end.astype(np.int64) - sc.cam_start).sum())
        assert total > 0
        if self.rs:
            R.tune("build_list_limit", total - 1)
            try:
                rc = self.rs.try_set_camera(sc.eye, sc.eye_to_top_left, sc.left_to_right, sc.top_to_bottom, sc.pixel_size_inv)
            finally:
                R.tune("build_list_limit", 0xFFFFFFFF)
            assert rc == -3 and "limit" in R.last_error(), f"refused move: returned {rc} with {R.last_error()!r}, expected -3"

    def do_clone(self, subset):
        """An instance made like the scene from the scene's own description (the pose of creation or of the last update)."""
        if not self.rs:
            return
        sc = self.w.base
        tiles = np.arange(R.tile_count(sc.width, sc.height), dtype=np.uint32)[1:] if subset else None
        # (the scene's own description rebuilds its lists with the host builders when read, which takes seconds on the larger scene's
        # rooms: there the clone is described by the model's Scene of the same pose and shape)
        desc = self.rs.scene if self.w.name == SMALL else self.w.state(self.described_pose, self.shape)
        c = R.ResidentScene(desc, 0, tiles, like=self.rs)
        try:
            S = self.samples  # a clone starts with the default window, whatever its model has, and renders the default window's frame
            assert c.sample_window()["next"] == dict(total=S, first=0, divisor=S, accumulate=0, advance=0), c.sample_window()
            self.same_bound(c, self.shape, "the clone's clip bound")
            c.render()
            got = [np.asarray(p).reshape(sc.height, sc.width) for p in c.readback()]
            mine = np.ones((sc.height, sc.width), bool)
            if subset:
                mine[:R.TILE, :R.TILE] = False  # tile 0 is not the clone's
                refusal(c.temporal, "every tile of the image", "temporal on a tile subset")
            for ch, g, x in zip("RGB", got, self.w.planes(self.described_pose, self.shape)):
                differs(g, np.where(mine, x, 0).astype(np.uint16), f"plane {ch} of the clone's frame")
        finally:
            c.close()


def describe(steps):
    return "; ".join(f"{i}: {k}" + ("" if a is None else f"({a})") for i, (k, a) in enumerate(steps))


def play(name, seed, part, last=None, report=None):
    """Plays one sequence on the device and stops at the first mismatch: one pass, nothing is tried again.  The scene is always closed
    (twins and clones close themselves).  report(step number, step, verdict) is called after every step."""
    seq = part_of(name, seed, part)
    steps = seq["steps"] if last is None else seq["steps"][:last + 1]
    w = world(name)
    rs = R.ResidentScene(w.state(*seq["start"]), 0)
    try:
        s = Session(w, seq["start"], rs)
        s.same_window("a fresh scene")
        for i, step in enumerate(steps):
            try:
                s.apply(step)
            except (AssertionError, RuntimeError) as e:
                if report:
                    report(i, step, f"MISMATCH: {e}")
                raise AssertionError(f"{name} seed {seed} part {part}, step {i} {step}: {e}\nstarted at {seq['start']}; steps so far: "
                                     f"{describe(steps[:i + 1])}") from e
            if report:
                report(i, step, "ok")
    finally:
        rs.close()
    return len(steps)
