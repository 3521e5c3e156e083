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
the header leaves undefined.

Looks.  The edit seeds (KINDS_EDIT, on class_textured_bumped, the base scene of the opaque-diffuse class) add the look to the state:
(light set, material set, (id variant, modulus)) from the small tables of look_parts, the model's Scene being the base scene's with
those fields replaced (edit_cases.twin_of).  A World per look keeps what depends on shading and shares the rest with the World of the
scene's own look.  The last rendered frame records its look: read_passes, denoise, temporal(denoise=) and the variance filter read
that frame's buffers and are that look's products, stale like a stale pose; what traces anew follows the look in effect; a continuing
frame is rendered onto the model's planes whatever look they came from, and the history arrays are carried across edits.  lights,
materials and ids check the path class (R.path_class of the model's Scene), the scene's description and word 21 of the shading rows;
refused_edit one illegal argument of EDIT_REFUSALS by code and text, with addresses and byte count unchanged -- except that the first
call that brings host ids, refused or not, makes their staging of 4 bytes per triangle (the header's Memory paragraph: ids are
checked on the device); matte_groups installs or frees the group table, which is state; mattes compares rtHipMatteDefaults with the
model's last window and the four outputs with matte_oracle, bit for bit, over the sample ids of the current pose and shape and the
table of the kind.  Whether a clone inherits the group table is left open by the header and is not checked.  Every sequence starts
from a fresh scene under the scene's own look.  The caps of these seeds: edit_caps, shows_its_edits and histories_cross.

Clamp and blurs.  The post seeds (KINDS_POST, on mirror_hall and, as a walk, on the four-tile axis_near_axis_mixed) add the temporal clamp
to the state -- None or (mode, gamma), off in a fresh scene and in every clone, whatever its parent's -- and two products of the last
frame that promise to change nothing.  clamp sets, changes or turns off the scene's clamp from CLAMP_SETTINGS, or hands over one
setting of CLAMP_REFUSALS, which returns -1 with its text and leaves the setting as it was; after every step of a post sequence the
scene's clamp (rs.temporal_clamp()) equals the model's.  While the clamp is on, temporal and temporal_variance equal
temporal_clamp_oracle.accumulate over the same inputs as before (the variance step with the history's moments, which are not clamped:
the model asserts on the oracles that count, moments and variance are the unclamped ones'); denoise= and filter= are applied after.
motion_blur (one of motion_blur_cases.SCENE_PARAMS) equals motion_blur_oracle.blur of the LAST RENDERED planes / 65535 along the flow of
the CURRENT state against the model's mark -- a stale frame keeps its colour under the new flow --, rgb bit for bit and the planes
quantised; it is refused without a mark, renders a frame first where the scene has none, and leaves the mark where it was
(same_mark against the mark's state), the history and the moments alone, which the later steps prove.  dof (one of
dof_cases.SCENE_PARAMS) equals dof_oracle.blur of the model's planes / 65535 by the depth pass of the frame's twin, under the frame's
window, the focus being the median of the depths that hit, handed to both sides as one number; it is refused without the depth pass
in the mask, renders a frame first where there is none under the mask in effect (as read_passes does), gives the old frame's product
for a stale pose or shape, and changes nothing.  Without a device the model takes the depth pass from its definition (oracle_depth),
so that tests/test_session.py can measure the blurs and compare the model with the feature tests' own chains.  The draw of a passes
step favours masks with the depth pass (MASKS_POST), the draw of a clamp step looks one kind ahead (Lite.upcoming) so that a temporal
step directly follows the clamp being turned off over a history made under it; the caps: POST_FACTS and post_caps.

Layouts.  Under default tuning the small images render round 1 ordered and cut and every later round appended, and almost every frame
of a sequence is the first after some change: what the product keeps between the frames of an unchanged scene -- the launch plan
(Group::plan, planRounds), the placement tables and their stamps (rt_frame_plan.h, round_goes_direct), control words left clean by a
planned batch, the tile groups' copies, several sample batches -- is never live while the operations run.  So 58 sequences of
existing seeds (LAYOUT_SEEDS) are played once more under a layout (LAYOUTS: RT_* variables set in os.environ while the scene, its
clones and twins are created), and there every frame whose repetition is idempotent in the model (settles: the window neither
advances nor continues, wavefront pipeline) is rendered three times, a clone's too: each read-back equals the planes the model has
for the step, the second and third are not rendered again, and the last reports the placement the layout promises (Session.placed:
under direct and direct_unsplit every trace round of a frame in the opaque-diffuse class placed directly and none scattered, in the
general class all scattered; under cut all scattered; under groups nothing direct and round 1 scattered once per tile group and
sample batch, which is how the batch count is asserted).  The model is untouched by the repeats -- window_last, history, mark and
tile buffer are what one frame leaves --, so every later step checks what the step after a settled frame left behind.  Other frames
(advancing and continuing windows, the megakernel) are single frames between the settled ones.  COUNTS_LAYOUT holds what that
exercises.  Kinds that a layout's sequences never put between a settled frame and a later frame (LAYOUT_UNCOVERED): clamp,
motion_blur and dof under every layout (no post seed is played under one); under direct_unsplit also mark, window and lights; under
cut also lights; under groups also denoise, lights, materials, ids, refused_edit, matte_groups and mattes."""
import collections
import ctypes
import os

import numpy as np

import ao_oracle
import bake_oracle
import camera_cases as CC
import denoise_oracle as D
import dof_cases as DC
import dof_oracle as DO
import edit_cases as EC
import geometry_cases as GC
import matte_oracle as MA
import motion_blur_cases as BC
import motion_blur_oracle as BO
import motion_cases as MC
import motion_oracle as MO
import oracle_lib as O
import prep_oracle as P
import query_cases as Q
import sample_window_cases as WC
import scenarios
import temporal_clamp_cases as TCC
import temporal_clamp_oracle as CO
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
# The edit seeds of a scene draw from KINDS_EDIT: scene edits and mattes beside everything else (a circuit of 25 * 25 + 1 = 626 steps).
KINDS_EDIT = KINDS_WIDE + ("lights", "materials", "ids", "refused_edit", "matte_groups", "mattes")
# The post seeds of a scene draw from KINDS_POST: the temporal clamp, which is state, and the two blurs of the last frame, which promise to
# change none (a circuit of 22 * 22 + 1 = 485 steps).
KINDS_POST = KINDS_WIDE + ("clamp", "motion_blur", "dof")
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
# post_circuits / post_walks: the seeds that draw from KINDS_POST.  axis_near_axis_mixed is 5 x 5 blur tiles of 32 pixels over its four scene
# tiles, so its post walk runs the blurs' neighbourhood maxima on interior tiles and their scene gathers with slot > 0 and tilesX > 1;
# post_walk_cut: that walk is cut shorter than the wide walk (see COUNTS_POST).
SCENES = {"mirror_hall": dict(size=(24, 16), samples=2, circuits=(1, 2), walks=(101, 102), wide_circuits=(4,), wide_walks=(103,),
                              post_circuits=(36,), post_walks=(118,), shapes=GC.SEQUENCE, cut=40),
          "axis_near_axis_mixed": dict(size=(136, 132), samples=2, circuits=(3,), walks=(), wide_circuits=(), wide_walks=(106,),
                                       post_walks=(118,), post_walk_cut=16,
                                       shapes=tuple(n for n in GC.SEQUENCE if n != "translate"), cut=25, shape_steps=2, walk_cut=31),
          # class_textured_bumped is the one base scene of the opaque-diffuse class (six materials with one-texel height maps, a fifth
          # of the triangles without a material, one tube light, smooth normals); its seeds draw from KINDS_EDIT, and an edit walks
          # it into the general class and back (LIGHT_SETS, MATERIAL_SETS).  Cropped as mirror_hall is.  It keeps every pose and shape:
          # no state is empty.  min_hit: the soup is sparse (0.35..0.54 of the centre rays hit from the four poses outside it) and from
          # `inside` more than half of it lies behind the eye, where 0.11..0.21 hit -- 42 pixels and more of the 384, which temporal,
          # motion and matte steps still have answers for; motion_cases.MIN_HIT (0.2) was sized for rooms and halls.
          "class_textured_bumped": dict(size=(24, 16), samples=2, circuits=(), walks=(), wide_circuits=(), wide_walks=(),
                                        edit_circuits=(21,), edit_walks=(110,), shapes=GC.SEQUENCE, cut=40, min_hit=0.1)}
# A scene's number in the generators' keys (the order the scenes were added in: a new scene leaves the older ones' draws alone).
SCENE_KEY = {"axis_near_axis_mixed": 0, "mirror_hall": 1, "class_textured_bumped": 2}
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
# The edit seeds (tests/test_session.py prints the figures and asserts the counts): 82 edits, every one changing the look; class
# crossings: 9 by lights to the general class and 6 back, 17 by materials to the general class and 8 back; frames directly after a
# camera / a shape step: 1 / 1 in the general class, 2 / 1 in the opaque-diffuse one; 9 clones in another class than the one of
# creation; 1 frame continues another look's buffer; 2 temporal steps and 1 variance step find a live history across a class change
# under max_history 32, 32 and 4: they blend it in in 1.000, 0.953 and 0.339 of the pixels and differ there from the answer over an
# empty history;
# 26 mattes (6 triangle, 13 material, 7 group; 1 more refused for want of a table), 10 with defaults, 9 of those under another
# window_last than the default; 4 before any frame, 2 group mattes after a shape step and 6 after an edit made since the table was
# installed, 9 material mattes after an ids step; 2 overflow into rest, 24 hold a pixel of two layers, 13 take another sample count
# than S.  The 24 edits that a frame shows change 0.094..0.578 of the oracle's pixels (floor: MIN_EDIT_CHANGED); all 11 pairs of
# consecutive mattes under different states or tables differ.  27 states visited, hit share 0.107..0.539, changed share 0.034..0.688
# over 53 moves.
COUNTS_EDIT = dict(sequences=19, steps=703)
# The post seeds (tests/test_session.py prints the figures and asserts the counts; every figure is the oracles', none the device's):
# over the three seeds (mirror_hall's circuit 36 in 14 sequences and its walk 118; axis_near_axis_mixed's walk 118 in 5 sequences of at
# most 16 steps -- cut as its wide walk is, at 31, its first half took 4.9 s on the device, above the sizing rule of
# tests/test_session_gpu.py) 8 temporal steps run under the clamp with a live history and max_history above 1 (5 + 2 + 1) and 3
# variance steps with live moments (2 + 1 + 0); 2 temporal steps with max_history above 1 directly follow the step that turned the
# clamp off over a history made under it (the circuit's and the small walk's); of 23 motion blurs 9 have a mark that differs from the
# current state (7 + 1 + 1), 9 blur a stale frame and 3 stand between two temporal steps with no reset and no variance step between,
# the second under max_history above 1; of 15 depths of field 3 follow a mask change with no frame between, 4 blur a frame of another
# window than the default and 5 a stale frame.  POST_SHARES: of the 22 accumulation steps under the clamp 11 find a live history
# under max_history above 1, and there the clamped oracle's colour differs from the unclamped oracle's in 0.265 of the pixels on
# average (0.000..0.607; in some pixel in 10 of the 11), while counts, moments and variance are the unclamped ones' bit for bit; the
# motion blurs gather in 0.391 of their pixels on average -- in all pixels of the 9 whose mark differs from the state, which change
# their frame, in none of the 14 whose mark is the state, which return it (a circuit holds the pairs (mark, motion_blur), (temporal,
# motion_blur) and (variance, motion_blur), and which steps lie between a mark and a blur is the circuit's order, not the draw's; every
# walk must hold a blur that gathers) --; every depth of field gathers in all pixels (the focus is the median depth, so every
# 32-pixel tile neighbours one out of focus) and changes its frame.  The test asserts half of each share.
COUNTS_POST = dict(sequences=20, steps=622)
POST_SHARES = dict(clamped=0.265, motion_blur_gathered=0.391, dof_gathered=1.000)
# The clamp's settings (None: off; every mode, gammas from 0, where the variance box is the mean itself) and the settings that
# rtHipTemporalClampCheck refuses, with a word of its text: a refused step returns -1 and leaves the setting as it was.
CLAMP_SETTINGS = (None,) + tuple((mode, gamma) for mode in TCC.MODES for gamma in (0.0, 0.5, 1.0, 2.5))
CLAMP_REFUSALS = (((4, 1.0), "mode 4"), ((0, 0.5), "mode 0"), ((3, -1.0), "gamma"), ((2, -0.25), "gamma"))
# The masks a post seed's passes step draws from: mostly with the depth pass, which the depth of field needs, and with both surface
# passes, which the denoisers need.
MASKS_POST = (31, SURFACE | R.PASS_DEPTH, 30, 7, 31, R.PASS_DEPTH, SURFACE, 0, SURFACE | R.PASS_DEPTH)
WINDOW_SIZES = (2, 3, 4)  # N / S of a drawn window
VARIANCE_FILTER = dict(iterations=2, spatial_below=2.0)
SMALL = "mirror_hall"  # AO and the bake are also compared with their numpy oracles here
# Reduced sequences of mismatches found by the circuits: name -> (scene, (start pose, start shape), steps).
# material_pass_after_ids (reduced from class_textured_bumped seed 21 part 14, step 35): read_passes after an ids edit, with no frame between, gave the
# NEW ids in the material pass beside the old frame's albedo -- ResidentScene.readback_passes looked the frame's triangles up in the
# description in effect.  It reads the description the frame was issued under now.
REGRESSIONS = {"material_pass_after_ids": ("class_textured_bumped", ("home", "home"),
                                           (("passes", 31), ("frame", None), ("ids", ((1, 6), "numpy")), ("read_passes", None)))}
# Layouts: the RT_* variables a sequence is played under once more (play(layout=); the Python stub turns them into rtHipTune calls
# when a scene is created), so that the state the product keeps between the frames of an unchanged scene -- the launch plan, the
# placement tables and their stamps, clean control words, the tile groups' copies -- is live while the operations run.
# direct: every trace round is ordered and uncut (test_place_direct_gpu.BASE_ENV); in the opaque-diffuse class planned frames place
# their rounds directly.  direct_unsplit: the class ORDERED logic kernel places round 2, not wf_shade_kernel<true>.  cut: every round
# ordered and cut, region B sized from the plan, the slices merge mid-frame (the entry of pipeline_modes.MODES); nothing may go direct.
# groups: three tile groups on the four-tile scene and one sample per batch, so a frame of S = 2 renders in two batches: by
# build_wavefront (rt_scene_parts.cpp) a path takes 1860 bytes under the default extra_factor, 116.25 MiB for the 65536 pixels of four
# tiles and 87.2 MiB for the three of a tile subset, so a budget of 100 MiB holds one sample of either and not two.
LAYOUTS = {"direct": {"RT_WF_SEG_RAYS": "1", "RT_WF_APPEND_RAYS": "0"},
           "direct_unsplit": {"RT_WF_SEG_RAYS": "1", "RT_WF_APPEND_RAYS": "0", "RT_WF_LOGIC_SPLIT": "0"},
           "cut": {"RT_WF_APPEND_RAYS": "0", "RT_WF_SEG": "24,24,24,24,24", "RT_WF_SEG_RAYS": "1,1,1,1", "RT_WF_SLICE_RAYS": "20000",
                   "RT_WF_SMALL_SLICES": "4"},
           "groups": {"RT_WF_GROUPS": "3", "RT_WF_STATE_MB": "100"}}
# (layout, scene, seed): the sequences played under a layout, all of existing seeds -- 18 + 1 + 8, 1, 11 + 1 and 16 + 2 sequences.
LAYOUT_SEEDS = (("direct", "class_textured_bumped", 21), ("direct", "class_textured_bumped", 110), ("direct", "mirror_hall", 1),
                ("direct_unsplit", "class_textured_bumped", 110), ("cut", "mirror_hall", 4), ("cut", "class_textured_bumped", 110),
                ("groups", "axis_near_axis_mixed", 3), ("groups", "axis_near_axis_mixed", 106))
SETTLED_FRAMES = 3  # under a layout a frame that can be rendered again is: the first may be watched, the others run from what it left
# What the sequences under a layout exercise, by the light model alone (layout_facts; tests/test_session.py prints the figures and asserts
# them per seed, and per layout what they add up to): the frames of the sequences' own scenes, settled (rendered SETTLED_FRAMES times)
# and single, the settled ones by path class; the clones, whose frames are settled as well; and per kind of step -- one that the
# state refuses apart -- how often it lies between a settled frame and a later frame of its sequence.  Over the 58 sequences the
# device renders 28 + 4 + 23 = 55 settled frames under direct, 26 of them in the opaque-diffuse class, 4 under direct_unsplit,
# 18 + 4 under cut and 33 + 3 under groups, and as many clone frames as there are clones.
COUNTS_LAYOUT = {
    ("class_textured_bumped", 21): dict(
        sequences=18, steps=643, settled=28, single=18, settled_class=22, settled_general=6, clones=25,
        between={'ao': 5, 'bake': 4, 'camera': 7, 'clone': 6, 'denoise': 3, 'denoise (refused)': 6, 'frame': 9, 'ids': 6, 'intersect': 5,
                 'lights': 10, 'mark': 6, 'materials': 13, 'matte_groups': 9, 'mattes': 6, 'mattes (refused)': 1, 'motion': 8,
                 'motion (refused)': 4, 'passes': 9, 'pipeline': 1, 'read_passes': 8, 'refused_camera': 9, 'refused_edit': 12,
                 'refused_update': 7, 'reset_temporal': 5, 'shape': 8, 'temporal': 8, 'temporal (refused)': 0, 'variance': 9, 'window': 12,
                 'window (refused)': 1}),
    ("class_textured_bumped", 110): dict(
        sequences=1, steps=60, settled=4, single=0, settled_class=4, settled_general=0, clones=1,
        between={'ao': 2, 'bake': 2, 'camera': 2, 'clone': 1, 'denoise': 2, 'denoise (refused)': 1, 'frame': 1, 'ids': 2, 'intersect': 2,
                 'materials': 2, 'matte_groups': 1, 'mattes': 2, 'motion': 1, 'motion (refused)': 0, 'passes': 3, 'pipeline': 1,
                 'pipeline (refused)': 1, 'read_passes': 2, 'refused_camera': 3, 'refused_edit': 2, 'refused_update': 1, 'reset_temporal': 3,
                 'shape': 2, 'temporal': 3, 'variance': 6}),
    ("mirror_hall", 1): dict(
        sequences=8, steps=297, settled=23, single=3, settled_class=0, settled_general=23, clones=17,
        between={'ao': 10, 'bake': 9, 'camera': 9, 'clone': 13, 'denoise': 3, 'denoise (refused)': 8, 'frame': 9, 'intersect': 12, 'mark': 11,
                 'motion': 9, 'motion (refused)': 3, 'passes': 10, 'pipeline': 16, 'read_passes': 10, 'refused_camera': 9,
                 'refused_update': 12, 'reset_temporal': 13, 'shape': 9, 'temporal': 10, 'temporal (refused)': 0}),
    ("mirror_hall", 4): dict(
        sequences=11, steps=372, settled=18, single=15, settled_class=0, settled_general=18, clones=19,
        between={'ao': 3, 'bake': 9, 'camera': 4, 'clone': 6, 'denoise': 4, 'denoise (refused)': 3, 'frame': 7, 'intersect': 5, 'mark': 7,
                 'motion': 4, 'motion (refused)': 0, 'passes': 4, 'passes (refused)': 0, 'pipeline': 3, 'pipeline (refused)': 1,
                 'read_passes': 9, 'refused_camera': 4, 'refused_update': 7, 'reset_temporal': 4, 'shape': 6, 'temporal': 5,
                 'temporal (refused)': 1, 'variance': 4, 'variance (refused)': 0, 'window': 4, 'window (refused)': 0}),
    ("axis_near_axis_mixed", 3): dict(
        sequences=16, steps=305, settled=33, single=2, settled_class=0, settled_general=33, clones=18,
        between={'ao': 10, 'bake': 8, 'camera': 10, 'clone': 9, 'denoise': 0, 'denoise (refused)': 8, 'frame': 4, 'intersect': 6, 'mark': 10,
                 'motion': 12, 'motion (refused)': 2, 'passes': 10, 'pipeline': 8, 'read_passes': 5, 'refused_camera': 7,
                 'refused_update': 9, 'reset_temporal': 10, 'shape': 8, 'temporal': 8, 'temporal (refused)': 0}),
    ("axis_near_axis_mixed", 106): dict(
        sequences=2, steps=61, settled=3, single=3, settled_class=0, settled_general=3, clones=3,
        between={'ao': 1, 'bake': 1, 'camera': 1, 'clone': 0, 'frame': 2, 'intersect': 1, 'mark': 1, 'motion': 0, 'passes': 0, 'pipeline': 1,
                 'read_passes': 2, 'refused_camera': 1, 'refused_update': 0, 'reset_temporal': 2, 'shape': 1, 'temporal': 4,
                 'temporal (refused)': 0, 'variance': 2, 'variance (refused)': 0, 'window': 2})}
# The kinds that no step of a layout's sequences puts between a settled frame and a later frame (refused steps not counted; the module
# docstring lists them): no post seed is played under a layout, direct covers everything else (circuit 21 alone does), the walk 110
# draws no lights, mark or window step, and the larger scene has no edit seed and its circuit 3 no denoise step in that position.
KINDS_ALL = KINDS_EDIT + KINDS_POST[len(KINDS_WIDE):]
LAYOUT_UNCOVERED = {"direct": ("clamp", "motion_blur", "dof"),
                    "direct_unsplit": ("mark", "window", "lights", "clamp", "motion_blur", "dof"),
                    "cut": ("lights", "clamp", "motion_blur", "dof"),
                    "groups": ("denoise", "lights", "materials", "ids", "refused_edit", "matte_groups", "mattes", "clamp", "motion_blur", "dof")}


def flags(mask):
    return dict(alpha=bool(mask & R.PASS_ALPHA), depth=bool(mask & R.PASS_DEPTH), triangle=bool(mask & R.PASS_TRIANGLE),
                normal=bool(mask & R.PASS_NORMAL), albedo=bool(mask & R.PASS_ALBEDO))


# ---- looks: what the edits of a resident scene replace ------------------------------------------------------------------------------
# A look is (light set, material set, (id variant, modulus)): the ids in effect are the variant's folded into 0 .. modulus - 1 with every
# -1 kept (edit_cases.fold).  The modulus is the material count of the set the ids were handed over for: tables that come alone leave
# the resident ids as they are, so it may be smaller than the count of the set in effect.  The tables are small and fixed, so that the
# oracle's products and the twins of a look are shared between steps.
LIGHT_SETS = ("own", "none", "sun", "sun_spot", "many65")  # sun_spot and many65 (past the logic kernel's 64-light split): general class
MATERIAL_SETS = ("own", "hall", "lambert2")  # hall: mirror_hall's four, reflective and transparent: general class
ID_VARIANTS = (0, 1)  # the scene's own ids; a permutation of them with more -1 mixed in
EDIT_REFUSALS = ("shrink", "bad_first", "bad_last", "host_pointer", "neither", "past_atlas", "65536_lights", "null_light_array")
REJECTED = "a triangle uses a material >= materialCount"
MATTE_KINDS = ("triangle", "material", "group")
MATTE_LAYERS = (2, 4, 8)
MATTE_SELECT = (0, 2, 5)  # ids selected: the most frequent of the answer, one that nothing hits and the most frequent again
GROUP_SEEDS = (5, 6, 7)
_look_parts = {}


def default_look(name):
    return ("own", "own", (0, look_parts(name)["counts"]["own"]))


def look_parts(name):
    """The tables of scene `name`: {"lights": set -> six arrays, "materials": set -> tables and atlas, "counts": set -> material count,
    "ids": variant -> [T] int32 before folding}."""
    if name not in _look_parts:
        base = getattr(scenarios, name)()
        T = base.triangle_count
        rng = np.random.default_rng(77)
        own = np.asarray(base.tri_material, np.int32)
        mixed = np.where(rng.random(T) < 0.15, -1, own[rng.permutation(T)]).astype(np.int32)
        lights = dict(own=EC.lights_of(base), none=EC.lights_of([]), sun=EC.lights_of(EC.ONE_SUN), sun_spot=EC.lights_of(EC.ONE_SUN + [EC.SPOT]),
                      many65=EC.lights_of(EC.many_lights(65, 2)))
        mats = dict(own=EC.materials_of(base), hall=EC.materials_of(scenarios.mirror_hall()),
                    lambert2=EC.materials_of([scenarios._lambert(), scenarios._lambert(color=(220, 40, 30))]))
        counts = {k: int(np.asarray(v["mat_size"]).reshape(-1, 2).shape[0] // 5) for k, v in mats.items()}
        _look_parts[name] = dict(lights=lights, materials=mats, counts=counts, ids={0: own, 1: mixed})
    return _look_parts[name]


def look_ids(name, ids):
    """The [T] int32 material ids of a look's id part (variant, modulus)."""
    return EC.fold(look_parts(name)["ids"][ids[0]], ids[1])


_look_class = {}


def look_class(name, look):
    """R.path_class of the scene under the look (decided on the host from the tables alone)."""
    if (name, look[:2]) not in _look_class:
        parts = look_parts(name)
        sc = EC.twin_of(getattr(scenarios, name)(), lights=parts["lights"][look[0]], materials=parts["materials"][look[1]])
        _look_class[name, look[:2]] = R.path_class(sc)
    return _look_class[name, look[:2]]


def group_table(T, seed):
    """Many triangles in few groups, some in none, some group ids above T (the table of tests/test_mattes_gpu.py)."""
    rng = np.random.default_rng(seed)
    table = rng.integers(0, 5, T).astype(np.uint32)
    table[rng.random(T) < 0.15] = NONE
    big = rng.random(T) < 0.2
    table[big] = rng.choice(np.array([T + 1, 1_000_000, 0xFFFFFFFE], np.uint32), int(big.sum()))
    return table


def selection(g, n):
    """n ids to select from the samples' ids g: the most frequent ones, then an id nothing hits, then the most frequent again."""
    if not n:
        return []
    hit = g[g != NONE]
    values, counts = np.unique(hit, return_counts=True)
    ranked = [int(v) for v in values[np.argsort(-counts, kind="stable")]]
    unhit = next(t for t in range(1 << 20) if t not in set(ranked))
    return (ranked[:max(n - 2, 1)] + [unhit] + ranked[:1])[:n]


# ---- the oracle's view of a base scene's 5 x 7 states -------------------------------------------------------------------------------
class World:
    """The states of a base scene under one look (None: the scene as scenarios.py makes it).  The World of another look shares what
    depends on geometry and camera alone -- grids, lists, walks, flows, sample ids and all of prep_oracle's records but the id word --
    with the World of the scene's own look, and keeps what depends on shading: the Scenes, the planes and the window frames."""

    def __init__(self, name, look=None):
        self.name, self.size, self.look = name, SCENES[name]["size"], look
        self.key = name if look is None else (name, look)  # (what a twin of this World's Scenes is cached under)
        self.geo = self if look is None else world(name)
        self.base = MC.base_scene(name, self.size) if look is None else self.dressed(self.geo.base)
        self.width, self.height = self.base.width, self.base.height
        self._shape, self._state, self._planes, self._trace, self._flow, self._prep, self._window = {}, {}, {}, {}, {}, {}, {}
        self._ids, self._depth, self._blurred = {}, {}, {}
        assert self.base.sample_count == SCENES[name]["samples"]

    def dressed(self, sc):
        """The Scene with this World's lights, materials and ids in place of its own."""
        parts = look_parts(self.name)
        return EC.twin_of(sc, lights=parts["lights"][self.look[0]], materials=parts["materials"][self.look[1]],
                          ids=look_ids(self.name, self.look[2]))

    def shape_scene(self, shape):
        if shape not in self._shape:
            if self.look is not None:
                self._shape[shape] = self.dressed(self.geo.shape_scene(shape))
                return self._shape[shape]
            sc = GC.with_arrays(self.base, *GC.arrays(self.base, shape), lists=False)
            sc.box_min, sc.grid_start, sc.grid_list = O.oracle_scene_grid(sc)
            self._shape[shape] = sc
        return self._shape[shape]

    def prep(self, shape):
        """prep_oracle's records and dense view of the shape (seconds on the larger scene's grid, and a circuit updates to the same
        few shapes many times).  Under a look: the shape's, with word 21 of the shading rows -- the material id -- the look's."""
        if shape not in self._prep:
            if self.look is not None:
                rec, shade, view = self.geo.prep(shape)
                shade = np.array(shade, copy=True)
                shade.view(np.int32)[:, 21] = look_ids(self.name, self.look[2])
                self._prep[shape] = (rec, shade, view)
                return self._prep[shape]
            self._prep[shape] = prep_of(self.shape_scene(shape))
        return self._prep[shape]

    def sample_ids(self, pose, shape, N, f, C_):
        """matte_oracle.sample_ids of the state under the window {N, f} with C samples: the primary hit of every sample."""
        if self.look is not None:
            return self.geo.sample_ids(pose, shape, N, f, C_)
        if (pose, shape, N, f, C_) not in self._ids:
            self._ids[pose, shape, N, f, C_] = MA.sample_ids(self.state(pose, shape), N, f, C_)
            self._ids[pose, shape, N, f, C_].setflags(write=False)
        return self._ids[pose, shape, N, f, C_]

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
            self._state[pose, shape] = (CC.posed(self.shape_scene(shape), pose) if self.look is None
                                        else self.dressed(self.geo.state(pose, shape)))
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
        if self.look is not None:
            return self.geo.trace(pose, shape)
        if (pose, shape) not in self._trace:
            self._trace[pose, shape] = MO.trace(self.state(pose, shape))
        return self._trace[pose, shape]

    def flow(self, cur, ref):
        """motion_oracle.motion of state `cur` against the reference state `ref` ((pose, shape) each)."""
        if self.look is not None:
            return self.geo.flow(cur, ref)
        if (cur, ref) not in self._flow:
            self._flow[cur, ref] = MO.project(self.state(*cur), self.state(*ref), self.trace(*cur))
        return self._flow[cur, ref]

    def depth(self, pose, shape, total, first):
        """The depth pass of a frame of the state that renders sample ids first+1 .. of a sequence of `total`, by its definition
        (oracle_depth): what the model without a device blurs by; on the device the twin's pass is read instead."""
        if self.look is not None:
            return self.geo.depth(pose, shape, total, first)
        if (pose, shape, total, first) not in self._depth:
            self._depth[pose, shape, total, first] = oracle_depth(self.state(pose, shape), total, first)
            self._depth[pose, shape, total, first].setflags(write=False)
        return self._depth[pose, shape, total, first]

    def motion_blurred(self, planes, cur, ref, variant):
        """motion_blur_oracle.blur (with its parts) of the planes / 65535 along the flow of `cur` against `ref` under
        motion_blur_cases.SCENE_PARAMS[variant]; cached per what the planes hold, so that a module's fixture can make it beforehand."""
        key = (cur, ref, variant) + tuple(np.asarray(p).tobytes() for p in planes)  # (the bytes themselves: the planes are small)
        if key not in self._blurred:
            flow = self.flow(cur, ref)
            colour = np.stack(planes, -1).astype(F32) / F32(65535.0)
            self._blurred[key] = BO.blur(colour, flow["motion"], flow["t"], **BC.SCENE_PARAMS[variant], with_parts=True)
        return self._blurred[key]


def oracle_depth(sc, total, first):
    """[H, W] f32: the DEPTH pass as include/raytrace_hip.h defines it, for a frame whose first sample has id first + 1 in a sequence
    of `total`: that sample's ray (seed p * total + first + 1, LR jitter, then TB) against the pixel's camera list in order with a
    running closest hit, t * |d|; +inf on a miss.  (sample_window_cases.window_passes restates every pass; this is its depth alone.)"""
    C = ctypes
    L = O.oracle()
    f3 = C.c_float * 3
    W, H = sc.width, sc.height
    eye = f3(*[float(v) for v in np.asarray(sc.eye, F32)[:3]])
    tl, lr, tb = (np.asarray(v, F32)[:3] for v in (sc.eye_to_top_left, sc.left_to_right, sc.top_to_bottom))
    corners = np.asarray(sc.vertex, F32)[np.asarray(sc.tri_index)[:, :3], :3]
    verts = {}
    depth = np.full(H * W, np.inf, F32)
    t, l1, l2 = C.c_float(), C.c_float(), C.c_float()
    start, end, cam = np.asarray(sc.cam_start), np.asarray(sc.cam_end), np.asarray(sc.cam_list)
    for p in range(H * W):
        state = C.c_uint64(p * total + first + 1)
        kx = F32(p % W) + F32(L.rt_oracle_randf(C.byref(state), 0.0, 1.0))
        ky = F32(p // W) + F32(L.rt_oracle_randf(C.byref(state), 0.0, 1.0))
        d = tl.copy()
        d = d + lr * kx
        d = d + tb * ky
        dc = f3(*[float(v) for v in d])
        best_t = None
        for c in cam[int(start[p]):int(end[p])]:
            c = int(c)
            if c not in verts:
                verts[c] = [f3(*[float(v) for v in corner]) for corner in corners[c]]
            a, b, cc = verts[c]
            if L.rt_oracle_ray_triangle(eye, dc, 0.0, float(np.inf if best_t is None else best_t), a, b, cc, C.byref(t), C.byref(l1), C.byref(l2)):
                best_t = F32(t.value)
        if best_t is not None:
            depth[p] = best_t * np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    return depth.reshape(H, W)


_worlds = {}


def world(name, look=None):
    """The World of the scene under `look`; the scene's own look is the World of no look."""
    if look is not None and look == default_look(name):
        look = None
    key = name if look is None else (name, look)
    if key not in _worlds:
        _worlds[key] = World(name, look)
    return _worlds[key]


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
    key = (w.key, pose, shape, mask) + (() if (total, first) == (samples, 0) else (total, first))
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


def settles(window, pipeline):
    """Whether rendering the frame of `window` again is idempotent in the model, so that under a layout the device renders it
    SETTLED_FRAMES times: the window does not advance and the frame does not continue from the tile buffer (every frame of it is the
    same frame), on the wavefront pipeline (the megakernel keeps no plan and no table).  The one rule of the model's count
    (Lite.render_frame, tests/test_session.py) and of the device (Session.on_device)."""
    N, f, D, acc, adv = window
    return pipeline == R.PIPELINE_WAVEFRONT and not adv and not (acc and f > 0)


class CapLog:
    """What the caps of the edit seeds ask about a sequence, kept beside the light state: nothing but the caps and the draw's
    steering towards them reads it."""

    def __init__(self):
        # ("edit", kind, class before, class after, look before, look after), ("mattes", facts), ("clone", whether in another class
        # than the one of creation), ("temporal" | "variance", Lite.across)
        self.events = []
        self.prev = None  # the kind of the step before
        self.pending = None  # (look before, look after) of the last edit, until a frame shows it or another edit follows
        self.hist_classes = None  # the classes of the frames the live history holds; None: no history
        self.moments_live = False  # the history's moments are live: the last of its steps was a variance step
        self.table_shape = self.table_edit = False  # a shape step / an edit was made since the group table was installed
        self.ids_step = False  # an ids step was made in this sequence


class Lite:
    def __init__(self, pose="home", shape="home", samples=2, name=None, post=False):
        self.pose, self.shape, self.mask, self.pipeline = pose, shape, 0, R.PIPELINE_WAVEFRONT
        # the post seeds (post: the steps may be of KINDS_POST): the temporal clamp, None or (mode, gamma), and what the caps of their draw
        # ask, as ("post", fact) events of self.log -- the history the accumulation keeps (None, or whether its last step ran under the
        # clamp and which kind it was), whether its moments are live, whether the step before turned the clamp off over a history made
        # under it, and whether a motion blur has been made since the last temporal step with no reset between
        self.post, self.clamp = post, None
        self.p_hist, self.p_moments, self.p_just_off, self.p_blurred = None, False, False, False
        self.upcoming = None  # (while a post seed is drawn: the kind of the step after the one being drawn, or None)
        # the edit seeds (name: the scene whose look tables the steps index): the look in effect and the one the last frame was
        # rendered under, the group table (the seed of group_table, or None), and what the caps of the draw ask (self.log)
        self.name = name
        self.look = self.look0 = default_look(name) if name else None
        self.frame_look, self.groups, self.log = None, None, CapLog()
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
        if kind == "mattes":
            return arg[0] == "group" and self.groups is None
        if kind == "clamp":
            return arg is not None and arg[0] == "refused"
        if kind == "motion_blur":  # (no shape of geometry_cases.SEQUENCE changes the triangle count, so the header's "reference made
            return self.mark is None  # for another triangle count" cannot occur: tests/test_session.py asserts it)
        if kind == "dof":
            return not self.mask & R.PASS_DEPTH
        return kind in ("refused_update", "refused_camera", "refused_edit")

    def renders(self, uses_passes):
        return self.frame is None or (uses_passes and self.frame[2] != self.mask)

    def cls(self, look=None):
        return look_class(self.name, look or self.look)

    def max_id(self):
        """The largest material id in effect."""
        return int(look_ids(self.name, self.look[2]).max())

    def after(self, step):
        """The look a successful edit step leaves."""
        kind, arg = step
        L, M, ids = self.look
        if kind == "lights":
            return (arg, M, ids)
        if kind == "materials":
            return (L, arg[0], arg[1] or ids)
        return (L, M, arg[0])

    def advance(self, step):
        """The step's effect on (pose, shape, mask, pipeline, frame, mark, updated) and, for the edit seeds, on the look and the group
        table; a refused step has none."""
        self._advance(step)
        self.log.prev = step[0]

    def _advance(self, step):
        kind, arg = step
        just_off, self.p_just_off = self.p_just_off, False
        if self.refuses(step) and kind != "clone":
            if kind == "mattes":
                self.log.events.append(("mattes", dict(kind=arg[0], refused=True)))
            return
        if self.post:
            self.post_facts(kind, arg, just_off)
        if kind in ("lights", "materials", "ids"):
            new = self.after(step)
            self.log.events.append(("edit", kind, self.cls(), self.cls(new), self.look, new))
            self.log.pending = (self.look, new)  # until the next frame or the next edit
            self.look, self.log.table_edit, self.log.ids_step = new, self.groups is not None, self.log.ids_step or kind == "ids"
        elif kind == "matte_groups":
            self.groups, self.log.table_shape, self.log.table_edit = arg, False, False
        elif kind == "mattes":
            S, last = self.samples, self.window_last
            table = None if arg[0] == "triangle" else self.look[2] if arg[0] == "material" else self.groups
            self.log.events.append(("mattes", dict(kind=arg[0], refused=False, defaults=arg[3] is None, before_frames=self.frame is None,
                                               state=(self.pose, self.shape), table=table,
                                               other_window=last is not None and last[:2] != (S, 0),
                                               group_after_shape=arg[0] == "group" and self.log.table_shape,
                                               group_after_edit=arg[0] == "group" and self.log.table_edit,
                                               material_after_ids=arg[0] == "material" and self.log.ids_step)))
        elif kind == "clone" and self.name:
            self.log.events.append(("clone", self.cls() != self.cls(self.look0)))
        if kind == "shape":
            self.log.table_shape = self.groups is not None
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
        elif kind == "clamp":
            self.clamp = arg
        if (kind == "frame" or (kind in ("read_passes", "denoise", "dof") and self.renders(True))
                or (kind in ("temporal", "variance") and self.renders(arg[0])) or (kind == "motion_blur" and self.renders(False))):
            self.render_frame()
        if kind in ("temporal", "variance"):
            self.mark = (self.pose, self.shape)
        if kind == "reset_temporal":
            self.log.hist_classes, self.log.moments_live = None, False
        if kind in ("temporal", "variance") and self.name:
            self.log.events.append((kind, self.across(kind, arg[1])))
            self.log.hist_classes = (self.log.hist_classes if self.blends(kind, arg[1]) else set()) | {self.cls(self.frame_look)}
            self.log.moments_live = kind == "variance"

    def post_facts(self, kind, arg, just_off):
        """What the caps of the post seeds ask about a step that is not refused, noted before it takes effect (POST_FACTS), and the
        light state they are counted from."""
        fact = lambda name: self.log.events.append(("post", name))  # noqa: E731
        if kind in ("temporal", "variance"):
            if self.clamp is not None and self.p_hist is not None and (kind == "temporal" or self.p_moments) and arg[1] > 1:
                fact(f"{kind}_clamped_live")  # under the clamp with a live history (a variance step: with live moments)
            # (max_history above 1 in all three: at 1 the history is not blended in, and neither clamp, mark nor history could show)
            if kind == "temporal" and just_off and self.log.prev == "clamp" and arg[1] > 1:
                fact("temporal_after_off")  # directly after the clamp was turned off, over a history made under it
            if kind == "temporal" and self.p_blurred and arg[1] > 1:
                fact("blur_between_temporal")  # a motion blur since the temporal step that made the history, no reset or variance step between
            self.p_hist, self.p_moments, self.p_blurred = (self.clamp is not None, kind), kind == "variance", False
        elif kind == "reset_temporal":
            self.p_hist, self.p_moments, self.p_blurred = None, False, False
        elif kind == "clamp":
            self.p_just_off = arg is None and self.clamp is not None and self.p_hist is not None and self.p_hist[0]
        elif kind == "motion_blur":
            fact("motion_blur")
            if self.mark != (self.pose, self.shape):
                fact("blur_mark_differs")  # the mark differs from the current state in pose or shape
            if self.frame is not None and self.frame[:2] != (self.pose, self.shape):
                fact("blur_stale")  # the colour of the old pose under the flow of the current one
            self.p_blurred = self.p_hist is not None and self.p_hist[1] == "temporal"
        elif kind == "dof":
            fact("dof")
            if self.frame is not None and self.frame[2] != self.mask:
                fact("dof_after_mask_change")  # the mask changed with no frame between: the step renders one first
            elif self.frame is not None and self.frame[:2] != (self.pose, self.shape):
                fact("dof_stale")  # the old frame's colour and depth
            if window_kind(self.window_next if self.renders(True) else self.window_last, self.samples) != "default":
                fact("dof_window")  # the frame it blurs was rendered under another window than the default

    def blends(self, kind, cap):
        """Whether a temporal or variance step made now can blend the history into its frame: there is one, a variance step finds its
        moments live (over stale ones it starts the history again), and max_history is above 1 -- at 1 every pixel's count is capped to
        1 and the output is the frame itself, as over an empty history, so what the step leaves holds that frame alone."""
        return self.log.hist_classes is not None and (kind == "temporal" or self.log.moments_live) and cap > 1

    def across(self, kind, cap):
        """Whether such a step, its frame rendered, runs with a live history across a class change: it can blend (blends) a history that
        holds a frame of another class than the frame's.  Whether a tap is accepted only the oracle knows (histories_cross)."""
        return bool(self.blends(kind, cap) and self.log.hist_classes - {self.cls(self.frame_look)})

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
                                complete=complete, settled=settles(win, self.pipeline)))
        if self.name:  # the class the frame runs in and the step it follows; whether it continues another look's buffer; the edit it shows
            self.frames[-1].update(cls=self.cls(), follows=self.log.prev, look=self.look,
                                   other_look=bool(acc and f > 0 and self.frame_look not in (None, self.look)), edit=self.log.pending)
            self.frame_look, self.log.pending = self.look, None
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
        masks = MASKS_POST if s.post else MASKS
        if s.pipeline == R.PIPELINE_MEGAKERNEL:
            return pick([m for m in masks if m]) if dare else 0
        return pick(masks)
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
        # (the post seeds: over a live history under the clamp, directly after it was turned off, or after a motion blur, a cap that
        # lets the history show, and with it the clamp, the setting turned off, or a mark or history that the blur moved)
        shows = s.post and s.p_hist is not None and (s.clamp is not None or s.p_blurred or s.p_just_off)
        return (bool(on), int(pick(MAX_HISTORY[1:] if shows else MAX_HISTORY)))
    if kind == "refused_update":
        return (pick(UPDATE_REFUSALS), pick([n for n in shapes if n != s.shape]))
    if kind == "refused_camera":
        return pick([p for p in POSES if p != s.pose])
    if kind == "clone":
        return bool(tiles > 1 and dare)
    if kind == "variance":
        on = rng.random() < 0.5 if s.mask & SURFACE == SURFACE else dare
        # (the edit seeds: over live moments of another class than the look's, a cap that lets the history show)
        # (the post seeds: likewise under the clamp over live moments)
        return (bool(on), int(pick(MAX_HISTORY[1:] if (s.name and s.log.moments_live and s.log.hist_classes - {s.cls()})
                                   or (s.post and s.clamp is not None and s.p_moments) else MAX_HISTORY)))
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
    if kind == "clamp":
        if dare:  # one setting that rtHipTemporalClampCheck refuses: returns -1 with its text and changes nothing
            setting, text = pick(CLAMP_REFUSALS)
            return ("refused", setting, text)
        # off again where a temporal step follows over a history made under the clamp, so that the step shows whether "off" took effect
        # (s.upcoming: the draw looks one kind ahead), and in some draws otherwise; else another setting than the one in effect
        if s.clamp is not None and ((s.upcoming == "temporal" and s.p_hist is not None and s.p_hist[0]) or rng.random() < 0.15):
            return None
        return pick([c for c in CLAMP_SETTINGS[1:] if c != s.clamp])
    if kind == "motion_blur":
        return int(rng.integers(len(BC.SCENE_PARAMS)))
    if kind == "dof":
        return int(rng.integers(len(DC.SCENE_PARAMS)))
    if s.name:
        return draw_edit(rng, pick, kind, s, dare)
    return None


def draw_edit(rng, pick, kind, s, dare):
    """The argument of a step of one of the kinds the edit seeds add, and of a bake there (a `material` filter in half of the steps).
    An edit always changes the look; about half of the lights and materials steps cross the class boundary where a set does."""
    counts = look_parts(s.name)["counts"]
    L, M, ids = s.look
    if kind == "bake":
        return int(rng.integers(counts[M])) if rng.random() < 0.5 else None
    if kind in ("lights", "materials"):
        at, sets = (0, LIGHT_SETS) if kind == "lights" else (1, MATERIAL_SETS)
        others = [v for v in sets if v != s.look[at]]
        cross = [v for v in others if s.cls(s.look[:at] + (v,) + s.look[at + 1:]) != s.cls()]
        # (a crossing is likelier out of the opaque-diffuse class, which most sets lead back to, and certain under a live history,
        # so that temporal and variance steps find frames of both classes in it)
        new = pick(cross) if cross and (s.log.hist_classes is not None or rng.random() < (0.7 if s.cls() else 0.4)) else pick(others)
        if kind == "lights":
            return new
        # ids come exactly where a resident id would be out of range for the new tables, and in four draws of ten otherwise
        brings = s.max_id() >= counts[new] or rng.random() < 0.4
        return (new, (int(pick(ID_VARIANTS)), counts[new]) if brings else None)
    if kind == "ids":
        return (pick([(i, counts[M]) for i in ID_VARIANTS if (i, counts[M]) != ids]), "numpy" if rng.random() < 0.5 else "torch")
    if kind == "refused_edit":
        while True:  # a variant that is legal in the current look is drawn again: tables of max_id materials need a material
            variant = pick(EDIT_REFUSALS)
            if variant != "shrink" or s.max_id() >= 1:
                return variant
    if kind == "matte_groups":
        if s.groups is not None and rng.random() < 0.25:
            return None
        return int(pick([g for g in GROUP_SEEDS if g != s.groups]))
    if kind == "mattes":
        if s.groups is None:
            what = "group" if dare else pick(MATTE_KINDS[:2])
        else:
            what = pick(MATTE_KINDS + ("group",))
        S, last = s.samples, s.window_last
        moved = last is not None and last[:2] != (S, 0)
        window = None
        if rng.random() >= (0.85 if moved else 0.25):  # explicit {N, f, C}, C unequal to S in three draws of four
            C_ = int(pick((1, S, 4, 8)))  # (with four and eight samples a pixel holds more ids than two layers take)
            N = C_ + int(rng.integers(0, 6))
            window = (N, int(rng.integers(0, N - C_ + 1)), C_)
        return (what, int(pick(MATTE_SELECT)), int(pick(MATTE_LAYERS)), window)
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


def _piece(rng, kinds, start, tiles, shapes, seen, samples=2, name=None, post=False):
    """Steps for `kinds` from a fresh scene at `start`, and what the caps ask about them: (steps, refusals after each step, temporal
    steps on an older frame, motion steps with camera and shape both changed, temporal steps, the warm ones among them, each as the
    index of the step; and of the variance steps [(index, warm, stale moments over a live history)])."""
    s, steps, refused, stale, mixed = Lite(*start, samples=samples, name=name, post=post), [], [], [], []
    alphabet = KINDS_POST if post else KINDS_EDIT  # (KINDS and KINDS_WIDE are the beginning of both)
    seen, hist, temporal, warm = set(seen), False, [], []
    moments, variance = False, []
    for i, k in enumerate(kinds):
        kind = alphabet[k]
        s.upcoming = alphabet[kinds[i + 1]] if post and i + 1 < len(kinds) else None
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
    key = [SCENE_KEY[name], seed, attempt]
    tiles = R.tile_count(*spec["size"])
    alphabet = kinds_of(name, seed)
    edit, wide, post = alphabet is KINDS_EDIT, alphabet is KINDS_WIDE, alphabet is KINDS_POST
    walk = seed in spec["walks"] + spec["wide_walks"] + spec.get("edit_walks", ()) + spec.get("post_walks", ())
    lite = dict(samples=spec["samples"], name=name if edit else None, post=post)
    k = len(alphabet)
    kinds = [int(v) for v in np.random.default_rng(key).integers(k, size=WALK)] if walk else eulerian(np.random.default_rng(key), k)
    limit = walk_limit(name, seed) if walk else spec["cut"]
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
                                                    **lite)
        for n in range(len(piece), 1, -1):
            if refused[n - 1] > MAX_REFUSED * n or (whole and n < len(piece)):
                continue
            if sum(k == "shape" for k, _ in steps[:n]) > spec.get("shape_steps", n):
                continue  # (an update's check of the device arrays takes over a second on the larger scene's 12.6 million pairs)
            s, now = Lite(*start, **lite), set(seen)
            for step in steps[:n]:
                s.advance(step)
                now |= {s.pose, s.shape}
            tail = rest(at + n - 1, (s.pose, s.shape), now)
            if tail is not None:
                return [dict(start=start, steps=steps[:n], stale=sum(i < n for i in st), mixed=sum(i < n for i in mx), seen=now,
                             temporal=sum(i < n for i in tp), warm=sum(i < n for i in wm), variance=[v for v in vr if v[0] < n],
                             frames=s.frames, events=s.log.events)] + tail
        return None

    out = rest(0, ("home", "home"), {"home"})
    if out is None:
        return None
    stale, mixed, seen = sum(q.pop("stale") for q in out), sum(q.pop("mixed") for q in out), set().union(*(q.pop("seen") for q in out))
    variance, frames = [v for q in out for v in q.pop("variance")], [q.pop("frames") for q in out]
    events = [q.pop("events") for q in out]
    if sum(q.pop("warm") for q in out) < MIN_WARM * sum(q.pop("temporal") for q in out):
        return None  # (too few temporal steps with a history to reproject: the accepting share could not reach a third)
    if wide and not wide_caps(frames, variance, walk):
        return None
    if edit and not (walk or (edit_caps(edit_facts(frames, events)) and shows_its_edits(name, frames, events)
                              and histories_cross(across_notes(name, out)))):
        return None  # (the caps of the edit seeds are the circuit's to meet: the walk adds to them)
    if post and not post_caps(post_counts(events), walk, tiles):
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


# What the caps of the post seeds count (Lite.post_facts notes each as it occurs, refused steps never): a temporal step under the clamp
# with a live history and max_history above 1; a variance step under the clamp with live moments and max_history above 1; a temporal
# step with max_history above 1 directly after the clamp was turned off, over a history whose last step ran under it; the blurs that
# are not refused; a motion blur whose mark differs from the current state in pose or shape; one of a stale frame; one between two
# temporal steps with no reset and no variance step between, the second with max_history above 1 (counted at that step); a depth of
# field after the mask changed with no frame between; one of a frame rendered under another window than the default; one of a stale
# frame.
POST_FACTS = ("temporal_clamped_live", "variance_clamped_live", "temporal_after_off", "motion_blur", "blur_mark_differs", "blur_stale",
              "blur_between_temporal", "dof", "dof_after_mask_change", "dof_window", "dof_stale")


def post_counts(events):
    """How often each of POST_FACTS occurs in Lite.log.events (one list per sequence)."""
    return {k: sum(e == ("post", k) for part in events for e in part) for k in POST_FACTS}


def post_caps(counts, walk, tiles):
    """What a post seed's draw must hold, so that over the post seeds together every one of POST_FACTS occurs at least twice
    (tests/test_session.py asserts that).  The circuit: each twice, but the temporal step directly after the clamp was turned off
    once -- a circuit holds the pair (clamp, temporal) once (the draw of a clamp step looks one kind ahead for it); the small scene's
    walk brings the second.  Every walk: a motion blur whose mark differs from the current state (one that gathers: with the mark at
    the state the blur returns its frame) and a depth of field that is not refused.  The larger scene's walk, where the blurs run on
    several tiles and the sequences are short: a temporal or variance step under the clamp with a live history, and a depth of field
    of a stale frame or under another window."""
    if not walk:
        return all(counts[k] >= (1 if k == "temporal_after_off" else 2) for k in POST_FACTS)
    if not (counts["blur_mark_differs"] >= 1 and counts["dof"] >= 1):
        return False
    if tiles == 1:
        return counts["temporal_after_off"] >= 1
    return counts["temporal_clamped_live"] + counts["variance_clamped_live"] >= 1 and counts["dof_stale"] + counts["dof_window"] >= 1


def edit_facts(frames, events):
    """What the caps of the edit seeds ask, counted from Lite.frames and Lite.log.events (one list per sequence each)."""
    frames = [f for part in frames for f in part]
    events = [e for part in events for e in part]
    edits = [e for e in events if e[0] == "edit"]
    mattes = [e[1] for e in events if e[0] == "mattes" and not e[1]["refused"]]
    defaults = [m for m in mattes if m["defaults"]]
    general = {R.PATH_CLASS_GENERAL: "to_general", R.PATH_CLASS_OPAQUE_DIFFUSE: "to_opaque_diffuse"}
    out = dict(edits=len(edits), same_look=sum(e[4] == e[5] for e in edits), clones_in_another_class=sum(e[1] for e in events if e[0] == "clone"),
               frames_on_another_look=sum(f["other_look"] for f in frames), temporal_across=sum(e[1] for e in events if e[0] == "temporal"),
               variance_across=sum(e[1] for e in events if e[0] == "variance"), mattes=len(mattes), mattes_defaults=len(defaults),
               mattes_defaults_other_window=sum(m["other_window"] for m in defaults),
               mattes_refused=sum(e[1]["refused"] for e in events if e[0] == "mattes"))
    for kind in ("lights", "materials"):
        for cls, word in general.items():
            out[f"{kind}_{word}"] = sum(e[1] == kind and e[2] != e[3] == cls for e in edits)
    for cls, word in ((R.PATH_CLASS_GENERAL, "general"), (R.PATH_CLASS_OPAQUE_DIFFUSE, "opaque_diffuse")):
        for prev in ("camera", "shape"):
            out[f"frames_{word}_after_{prev}"] = sum(f["cls"] == cls and f["follows"] == prev for f in frames)
    for k in MATTE_KINDS:
        out[f"mattes_{k}"] = sum(m["kind"] == k for m in mattes)
    for k in ("before_frames", "group_after_shape", "group_after_edit", "material_after_ids"):
        out[f"mattes_{k}"] = sum(m[k] for m in mattes)
    return out


def edit_caps(facts):
    """What the edit seeds' draw must hold (tests/test_session.py asserts it on the oracle, over the edit seeds together): every edit
    changes the look; each of the four class crossings -- by lights or by materials, to the general class or back -- at least twice; in
    each class a frame directly after a camera step and directly after a shape step; a clone made while the class is not the class of
    creation; a frame that continues from a buffer another look's frame filled; a temporal and a variance step with a live history
    across a class change (Lite.across: max_history above 1; histories_cross asks the oracle whether it shows); a matte of every
    kind, a group matte after a shape step and one after an edit made since the table was installed, a material matte after an ids step, a matte before any frame of its sequence, a group matte refused for want of a
    table, and a third of the mattes with defaults under another window_last than the default window's."""
    need = [k for k in facts if k.startswith("frames_") or k.startswith("mattes_") and k not in ("mattes_defaults", "mattes_defaults_other_window",
                                                                                                "mattes_refused")]
    need += ["clones_in_another_class", "temporal_across", "variance_across", "mattes_refused"]
    crossings = [k for k in facts if k.startswith("lights_") or k.startswith("materials_")]
    return (facts["same_look"] == 0 and all(facts[k] >= 1 for k in need) and all(facts[k] >= 2 for k in crossings)
            and 3 * facts["mattes_defaults_other_window"] >= facts["mattes_defaults"] > 0)


MIN_EDIT_CHANGED = 0.05  # of the pixels: the oracle's planes of the looks before and after an edit that a frame shows
_canon = {}


def matte_canon(name, state, kind, table):
    """The layers (K = 8, the default window) of the state's matte of `kind` under `table` (material: the id part of a look; group:
    the seed of group_table): what two consecutive matte steps are told apart by."""
    if (name, state, kind, table) not in _canon:
        w = world(name)
        S = w.base.sample_count
        tab = None if kind == "triangle" else MA.material_table(look_ids(name, table)) if kind == "material" else \
            group_table(w.base.triangle_count, table)
        m = MA.mattes(w.sample_ids(*state, S, 0, S), tab, [], 8, S)
        _canon[name, state, kind, table] = (m["layer_id"], m["layer_coverage"])
    return _canon[name, state, kind, table]


def edit_shares(name, frames):
    """For every frame that is the first after an edit: the share of the pixels in which the oracle's planes of the looks before and
    after the edit differ at the frame's state."""
    return [GC.changed_share(world(name, f["edit"][0]).planes(*f["state"]), world(name, f["edit"][1]).planes(*f["state"]))
            for part in frames for f in part if f.get("edit")]


def matte_pairs(name, events):
    """(consecutive matte steps of one sequence taken under different states or tables, those of them whose answers differ)."""
    pairs = same = 0
    for part in events:
        keys = [(e[1]["state"], e[1]["kind"], e[1]["table"]) for e in part if e[0] == "mattes" and not e[1]["refused"]]
        for a, b in zip(keys, keys[1:]):
            if a != b:
                pairs += 1
                same += all(np.array_equal(x, y) for x, y in zip(matte_canon(name, *a), matte_canon(name, *b)))
    return pairs, pairs - same


def shows_its_edits(name, frames, events):
    """Not vacuous, on the oracle: every edit that a frame shows changes MIN_EDIT_CHANGED of the pixels, and consecutive matte steps
    under different states or tables differ."""
    pairs, differing = matte_pairs(name, events)
    return all(v >= MIN_EDIT_CHANGED for v in edit_shares(name, frames)) and pairs == differing > 0


def across_notes(name, parts):
    """The model alone over the sequences `parts` of an edit seed: (kind, figures) of every temporal and variance step that runs with a
    live history across a class change (Session.note_across)."""
    out = []
    for q in parts:
        s = Session(world(name), q["start"], edit=True)
        for step in q["steps"]:
            s.apply(step)
        out += [n[1:] for n in s.notes if n[0] == "across"]
    return out


def histories_cross(notes):
    """Not vacuous, on the oracle: of the steps of across_notes one temporal and one variance step blend the history in in some pixels
    (used; count > 1) and give another answer than over an empty history, so a history wiped by an edit or a crossing shows."""
    return all(any(k == kind and f["blended"] > 0 and f["differs"] > 0 for k, f in notes) for kind in ("temporal", "variance"))


def walk_limit(name, seed):
    """The most steps a sequence of the walk seed may have: WALK (the walk is one sequence) unless the scene cuts its walks (walk_cut),
    its post walk shorter still where it says so (post_walk_cut)."""
    spec = SCENES[name]
    return spec.get("post_walk_cut" if seed in spec.get("post_walks", ()) and "post_walk_cut" in spec else "walk_cut", WALK)


def lite_of(name, seed, start):
    """The light state a sequence of the seed starts from."""
    return Lite(*start, samples=SCENES[name]["samples"], name=name if is_edit(name, seed) else None, post=is_post(name, seed))


def kinds_of(name, seed):
    """The alphabet of a seed: the one of the list its scene names it in; a regression plays the newest alphabet its scene has seeds
    of, so on a scene with edit seeds its steps index the look tables."""
    if seed in REGRESSIONS:
        return KINDS_EDIT if edit_seeds(name) else KINDS
    return (KINDS_EDIT if seed in edit_seeds(name) else KINDS_POST if seed in post_seeds(name)
            else KINDS_WIDE if seed in seeds_of(name, wide=True) else KINDS)


def is_edit(name, seed):
    """Whether the seed's steps index the scene's look tables."""
    return kinds_of(name, seed) is KINDS_EDIT


def is_post(name, seed):
    """Whether the seed's steps may be of KINDS_POST: the clamp is compared after every step."""
    return kinds_of(name, seed) is KINDS_POST


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
    """The scene's seeds: all of them, the wide ones (wide=True) or the oldest (wide=False); the edit seeds are edit_seeds'."""
    spec = SCENES[name]
    old, new = spec["circuits"] + spec["walks"], spec["wide_circuits"] + spec["wide_walks"]
    return old + new + edit_seeds(name) + post_seeds(name) if wide is None else new if wide else old


def edit_seeds(name):
    """The scene's seeds that draw from KINDS_EDIT."""
    return SCENES[name].get("edit_circuits", ()) + SCENES[name].get("edit_walks", ())


def post_seeds(name):
    """The scene's seeds that draw from KINDS_POST."""
    return SCENES[name].get("post_circuits", ()) + SCENES[name].get("post_walks", ())


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
            s = lite_of(n, seed, q["start"])
            out.append((s.pose, s.shape))
            for step in q["steps"]:
                s.advance(step)
                out.append((s.pose, s.shape))
    return list(dict.fromkeys(out))


def layout_parts():
    """(scene, seed, part, layout) of every sequence that is played under a layout (LAYOUT_SEEDS)."""
    return [(name, seed, part, layout) for layout, name, seed in LAYOUT_SEEDS for part in range(len(sequences(name, seed)))]


def step_key(s, step):
    """What a step counts as in layout_facts: its kind, a step that the state refuses apart ("temporal (refused)"); the kinds that are
    refusals themselves and a clone, whose subset only has its temporal() refused, under their own name."""
    kind = step[0]
    return kind + (" (refused)" if s.refuses(step) and kind != "clone" and not kind.startswith("refused_") else "")


def layout_facts(name, seed):
    """What playing the seed's sequences under a layout exercises, from the light model alone: sequences and steps; the frames of the
    sequences' own scenes (a clone's apart: it is settled too, but shows nothing of its parent's state) that are settled (settles)
    and single, the settled ones by path class; and per step_key how often a step lies between a settled frame and a later frame of
    its sequence -- the last frame of the steps before it is a settled one, so the step finds plan, tables and buffers live, and a
    later step renders a frame, which shows what the step left stale.  Every key that occurs is listed, also with 0."""
    out = dict(sequences=0, steps=0, settled=0, single=0, settled_class=0, settled_general=0, clones=0, between={})
    own = R.path_class(world(name).base)
    for q in sequences(name, seed):
        s, marks = lite_of(name, seed, q["start"]), []
        for step in q["steps"]:
            key, n = step_key(s, step), len(s.frames)
            s.advance(step)
            marks.append((key, s.frames[n:]))
        out["sequences"] += 1
        out["steps"] += len(marks)
        out["clones"] += sum(key == "clone" for key, _ in marks)
        for f in s.frames:
            out["settled" if f["settled"] else "single"] += 1
            if f["settled"]:
                out["settled_class" if f.get("cls", own) == R.PATH_CLASS_OPAQUE_DIFFUSE else "settled_general"] += 1
        frame_at = [i for i, (_, fs) in enumerate(marks) if fs]
        last = None  # the last frame of the steps before: what it left is what the step finds
        for i, (key, fs) in enumerate(marks):
            out["between"].setdefault(key, 0)
            out["between"][key] += bool(last is not None and last["settled"] and i < frame_at[-1])
            last = fs[-1] if fs else last
    out["between"] = dict(sorted(out["between"].items()))
    return out


def warm_wide(name):
    """The model alone over the scene's wide sequences: every window frame, flow and accumulation their checks read is made now (the
    caches are the World's), as World.warm does for the planes of the visited states."""
    for seed in seeds_of(name, wide=True) + edit_seeds(name) + post_seeds(name):
        for q in sequences(name, seed):
            s = Session(world(name), q["start"], edit=is_edit(name, seed), post=is_post(name, seed), warming=True)
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

    def __init__(self, w, start=("home", "home"), rs=None, edit=False, post=False, warming=False, layout=None, tally=None):
        super().__init__(*start, samples=w.base.sample_count, name=w.name if edit else None, post=post)
        self.warming = warming  # played to fill the World's caches only: what is not cached (the depth of field's oracle) is left out
        # the layout the scene was created under (a key of LAYOUTS, or None): frames that settle are rendered SETTLED_FRAMES times
        # (on_device); tally (a Counter, optional) takes what they reported, for the figures of tests/test_session_gpu.py
        self.layout, self.tally = layout, tally
        self.w, self.rs = w, rs  # (w: the World of the scene's own look, which holds what depends on geometry and camera alone)
        self.described_pose = start[0]
        self.planes = self.history = None
        self.moments = None  # the live moments [H, W, 2] of the history; None: stale (a temporal step wrote none) or absent
        self.staged = False  # a call has brought host ids: the scene holds their staging (4 bytes per triangle) from then on
        self.notes = []

    def here(self):
        return (self.pose, self.shape)

    @property
    def lw(self):
        """The World of the look in effect: what traces anew follows it."""
        return world(self.w.name, self.look) if self.name else self.w

    @property
    def fw(self):
        """The World of the look the last frame was rendered under: what reads the frame's buffers is that look's, stale or not."""
        return world(self.w.name, self.frame_look) if self.name else self.w

    def apply(self, step):
        kind, arg = step
        getattr(self, "do_" + kind)(arg) if arg is not None else getattr(self, "do_" + kind)()
        self.advance(step)
        if self.rs:
            self.same_window(f"after {kind}")
            if self.post:
                self.same_clamp(self.rs, self.clamp, f"after {kind}")

    # -- frames
    def do_frame(self):
        """The frame of window_next: the window oracle's, onto the model's planes where the frame continues from the tile buffer."""
        N, f, D, acc, adv = self.window_next
        onto = self.planes if acc and f > 0 else None
        assert onto is not None or not (acc and f > 0), "a frame continues before the sequence's first frame: the header leaves the buffer open"
        want = self.lw.window_planes(self.pose, self.shape, N, f, D, onto)  # (onto the model's planes, whatever look they came from)
        if self.rs:
            self.on_device(self.rs, want, settles(self.window_next, self.pipeline),
                           f"of the frame at {self.here()} under the window {self.window_next}")
        self.before, self.planes = self.planes, want

    def on_device(self, rs, want, settled, what, tiles=None):
        """Scene rs (the session's, or a clone) renders the frame whose planes the model has as `want`.  Without a layout, or where
        rendering it again is not idempotent (settles), once.  Under a layout SETTLED_FRAMES times, each a render / finish / readback
        compared with the same planes: the first may be watched or redone (a kept plan can be too short for a new window), the
        others are planned frames of an unchanged scene, which are deterministic and must not be redone; what the last one reports
        of its ordered rounds is what the layout says (placed).  tiles: how many rs holds (None: the image's)."""
        sc = self.w.base
        frames = SETTLED_FRAMES if self.layout and settled else 1
        for n in range(1, frames + 1):
            rs.render()
            redone = frames > 1 and rs.finish()
            which = f" (frame {n} of {frames} under the layout {self.layout})" if frames > 1 else ""
            for ch, g, x in zip("RGB", rs.readback(), want):
                differs(np.asarray(g).reshape(sc.height, sc.width), x, f"plane {ch} {what}{which}")
            assert n == 1 or not redone, f"the frame {what}{which} was rendered again: its plan was too short, and nothing had changed"
        if frames > 1:
            self.placed(rs, what, R.tile_count(sc.width, sc.height) if tiles is None else tiles)

    def placed(self, rs, what, tiles):
        """After a settled frame's last repeat: (ordered rounds placed directly, scatter launches) of rtHipTestPlaceLog against the
        trace rounds the frame issued (rtHipTestRoundLog's round count less the logic round that consumes the last answers), by
        round_goes_direct and issue_round (rt_frame_plan.h, rt_frame.cpp).
        direct, direct_unsplit: every trace round is ordered and uncut over 256 slices; in the opaque-diffuse class the frame before
        left a valid stamp of this window for each (a watched frame forgets all stamps and its scatter launches make new ones, a
        planned one scatters where a stamp does not match and records it), so all are placed and none is scattered; the general class
        scatters every one.  cut: every trace round is ordered and cut, so none is placed and each is scattered.  groups: round 1 alone
        is ordered (the later ones hold fewer rays than append_rays), and every tile group scatters it once per sample batch -- the
        scene has min(3, tiles) groups and one sample per batch (LAYOUTS), so a frame with a trace round reports 3 S launches: the
        batch count, as the library reports it; several batches never go direct (a stamp of theirs is not valid)."""
        traced = int(R.lib().rtHipTestRoundLog(rs.handle, None, 0)) - 1
        log, cls = rs.place_log(), rs.path_class()
        in_class = cls == R.PATH_CLASS_OPAQUE_DIFFUSE
        assert traced >= 0, f"the frame {what} reports {traced + 1} rounds"
        if self.layout in ("direct", "direct_unsplit"):
            want = (traced, 0) if in_class else (0, traced)
        elif self.layout == "cut":
            want = (0, traced)
        else:
            want = (0, min(3, tiles) * self.samples * min(traced, 1))
        if self.tally is not None:
            self.tally[self.layout, "class" if in_class else "general", "traced" if traced else "untraced",
                       "direct" if log[0] else "scattered" if log[1] else "neither"] += 1
        assert log == want, \
            f"the settled frame {what} under the layout {self.layout}: the place log is {log} with {traced} trace rounds in path class {cls}, expected {want}"

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
            assert_device_arrays(self.rs, want, f"device arrays after the update to {name}", self.lw.prep(name))
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
            got, want = self.rs.readback_passes(), twin(self.fw, *self.frame)["passes"]
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
            got, made = self.rs.denoise(**params), twin(self.fw, *self.frame)
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

    def do_bake(self, material=None):
        """The bake, in some steps of the edit seeds with a `material` filter, which reads the id word: the twin of the filter is
        keyed by the shape, the ids and the filter."""
        if self.rs and material is not None:
            key = (self.w.name, self.shape, self.look[2], material)
            if key not in _twin_bake:
                t = R.ResidentScene(self.lw.state("home", self.shape), 0)
                try:
                    _twin_bake[key] = t.bake_ambient_occlusion(16, 16, rays=4, dilate=2, material=material)
                finally:
                    t.close()
            got = self.rs.bake_ambient_occlusion(16, 16, rays=4, dilate=2, material=material)
            for k in ("ao", "triangle"):
                differs(got[k], _twin_bake[key][k], f"bake {k} of material {material} (against the twin)")
            covered = got["triangle"][got["triangle"] != NONE]
            assert (look_ids(self.name, self.look[2])[covered] == material).all(), f"the bake of material {material} covers another material's triangle"
        elif self.rs:
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
    def same_mark(self, what, state=None):
        """The reference camera is the camera of `state` (the current state: what a call that marks leaves)."""
        cam, sc = self.rs.motion_reference_camera(), self.w.state(*(state or self.here()))
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
        if self.clamp is None:
            acc = TO.accumulate(colour, flow["motion"], flow["prev_t"], flow["triangle"], hist, max_history=float(cap), with_taps=True)
        else:  # the scene's clamp is on: the clamped accumulation's colour and count
            acc = self.clamped("temporal", colour, flow, hist, cap)
        self.notes.append(("temporal", self.frame[:2] != self.here(), float(acc["used"].mean())))
        if self.name and self.across("temporal", cap):
            fresh = TO.accumulate(colour, flow["motion"], flow["prev_t"], flow["triangle"], TO.empty_history(self.w.height, self.w.width),
                                  max_history=float(cap))
            self.note_across("temporal", cap, acc["used"], acc, fresh, ("colour", "count"))
        if self.rs:
            shown = acc["colour"]
            if on:
                surf = twin(self.fw, *self.frame)["passes"]
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
        if self.clamp is None:
            acc = VO.accumulate(colour, flow["motion"], flow["prev_t"], flow["triangle"], hist, max_history=float(cap))
        else:  # the scene's clamp is on: the colour is clamped, the moments (taken with the history's) are not
            acc = self.clamped("variance", colour, flow, hist, cap)
        if not live:  # no history, or one that starts again: the frame itself
            assert (acc["count"] == 1.0).all() and (acc["variance"] == 0.0).all() and TO.same_bits(acc["colour"], colour).all()
        warm = self.history is not None and self.mark is not None and self.mark[1] == self.shape  # (as _piece counts it)
        self.notes.append(("variance", dict(stale=stale, warm=warm, live=live), float((acc["count"] > 1.0).mean())))
        if self.name and self.across("variance", cap):
            assert live
            fresh = VO.accumulate(colour, flow["motion"], flow["prev_t"], flow["triangle"], VO.empty_history(self.w.height, self.w.width),
                                  max_history=float(cap))
            self.note_across("variance", cap, acc["count"] > 1.0, acc, fresh, ("colour", "count", "moments", "variance"))
        if self.rs:
            shown = dict(colour=acc["colour"], variance=acc["variance"])
            if on:
                surf = twin(self.fw, *self.frame)["passes"]
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

    def clamped(self, kind, colour, flow, hist, cap):
        """temporal_clamp_oracle.accumulate under the model's clamp (with the moments where `hist` has some); notes the share of the
        pixels in which any output differs from the unclamped oracle's and, for a variance step, that the moments are the unclamped
        ones' bit for bit (the header: "the moments are not clamped")."""
        mode, gamma = self.clamp
        acc = CO.accumulate(colour, flow["motion"], flow["prev_t"], flow["triangle"], hist, max_history=float(cap), mode=mode, gamma=gamma)
        plain = (VO if kind == "variance" else TO).accumulate(colour, flow["motion"], flow["prev_t"], flow["triangle"], hist, max_history=float(cap))
        assert TO.same_bits(acc["count"], plain["count"]).all(), "the clamp changed a history length"
        if kind == "variance":
            assert TO.same_bits(acc["moments"], plain["moments"]).all() and TO.same_bits(acc["variance"], plain["variance"]).all()
        live = self.history is not None and (kind == "temporal" or self.moments is not None)
        differs_in = float(1.0 - TO.same_bits(acc["colour"], plain["colour"]).all(-1).mean())
        self.notes.append(("clamped", dict(kind=kind, live=live, cap=cap, clamp=self.clamp), differs_in))
        return acc

    def note_across(self, kind, cap, blended, acc, fresh, outputs):
        """A step with a live history across a class change (Lite.across): the share of the pixels that blend the history in, and the
        share in which an expected output differs from the one over an empty history -- what the step would give had an edit or a class
        crossing wiped the history."""
        same = np.ones(blended.shape, bool)
        for k in outputs:
            same &= TO.same_bits(acc[k], fresh[k]).reshape(blended.shape + (-1,)).all(-1)
        self.notes.append(("across", kind, dict(cap=cap, blended=float(np.mean(blended)), differs=float(1.0 - same.mean()))))

    def do_reset_temporal(self):
        if self.rs:
            self.rs.reset_temporal()
        self.history = self.moments = None

    # -- the temporal clamp: state of the scene; the accumulation steps above follow it
    @staticmethod
    def same_clamp(rs, clamp, what):
        want = None if clamp is None else dict(mode=clamp[0], gamma=clamp[1])
        got = rs.temporal_clamp()
        assert got == want, f"{what}: the scene's temporal clamp is {got}, the model's {want}"

    def do_clamp(self, arg=None):
        if not self.rs:
            return
        if self.refuses(("clamp", arg)):
            _, (mode, gamma), text = arg
            rc = int(R.lib().rtHipSceneSetTemporalClamp(self.rs.handle, ctypes.byref(R.temporal_clamp_params(mode, gamma))))
            assert rc == -1 and text in R.last_error(), f"refused clamp {(mode, gamma)}: returned {rc} with {R.last_error()!r}, expected -1 with {text!r}"
        elif arg is None:
            self.rs.set_temporal_clamp(None)
        else:
            self.rs.set_temporal_clamp(*arg)

    # -- the blurs of the last frame: they read the tile buffer (and the flow, or the depth word of the pass buffer) and change nothing,
    # which the later steps prove
    def do_motion_blur(self, variant):
        """rs.motion_blur: the LAST rendered frame's colour along the flow of the CURRENT state against the mark; the mark stays."""
        params = BC.SCENE_PARAMS[variant]
        if self.refuses(("motion_blur", variant)):
            if self.rs:
                refusal(lambda: self.rs.motion_blur(**params), "no motion reference", "motion_blur without a mark")
            return
        self.need_frame(False)
        parts = self.w.motion_blurred(self.planes, self.here(), self.mark, variant)
        colour = np.stack(self.planes, -1).astype(F32) / F32(65535.0)
        self.notes.append(("motion_blur", dict(stale=self.frame[:2] != self.here(), mark_differs=self.mark != self.here(),
                                               gathered=float(parts["gathered"].mean()),
                                               changed=not BO.same_bits(parts["out"], colour).all()), parts["out"]))
        if self.rs:
            got = self.rs.motion_blur(**params)
            differs(got["rgb"], parts["out"], f"motion_blur rgb {params} at {self.here()} against the mark at {self.mark}, frame of {self.frame[:2]}")
            for ch, g, x in zip("RGB", got["planes"], R.quantise(parts["out"])):
                differs(g, x, f"motion_blur plane {ch}")
            self.same_mark("motion_blur (the call does not mark)", self.mark)

    def do_dof(self, variant):
        """rs.depth_of_field: the last frame's colour by the depth pass of that frame, rendered first where there is none under the
        mask in effect (as read_passes); the focus is the median of the depths that hit, handed over as the number both sides use."""
        params = DC.SCENE_PARAMS[variant]
        if self.refuses(("dof", variant)):
            if self.rs:
                refusal(lambda: self.rs.depth_of_field(focus=1.0, **params), "depth pass", "depth_of_field without the depth pass")
            return
        self.need_frame(True)
        if self.warming:
            return
        pose, shape, mask, total, first = self.frame
        depth = twin(self.fw, *self.frame)["passes"]["depth"] if self.rs else self.w.depth(pose, shape, total, first)
        hit = depth[np.isfinite(depth) & (depth > 0)]
        assert hit.size, f"the frame at {self.frame[:2]} hit nothing"
        focus = float(np.median(hit))
        colour = np.stack(self.planes, -1).astype(F32) / F32(65535.0)
        parts = DO.blur(colour, depth, focus=focus, **params, with_parts=True)
        self.notes.append(("dof", dict(stale=self.frame[:2] != self.here(), window=window_kind(self.window_last, self.samples), focus=focus,
                                       gathered=float(parts["gathered"].mean()), changed=not DO.same_bits(parts["out"], colour).all()),
                           parts["out"]))
        if self.rs:
            got = self.rs.depth_of_field(focus=focus, **params)
            differs(got["rgb"], parts["out"], f"depth_of_field rgb {params}, focus {focus}, of the frame at {self.frame}")
            for ch, g, x in zip("RGB", got["planes"], R.quantise(parts["out"])):
                differs(g, x, f"depth_of_field plane {ch}")

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
        desc = self.rs.scene if self.w.name == SMALL or self.name else self.w.state(self.described_pose, self.shape)
        c = R.ResidentScene(desc, 0, tiles, like=self.rs)
        try:
            if self.name:  # the clone of an edited scene runs the class of a scene created with the look
                assert c.path_class() == R.path_class(self.lw.base), f"the clone's path class is {c.path_class()}, the look's {R.path_class(self.lw.base)}"
            S = self.samples  # a clone starts with the default window, whatever its model has, and renders the default window's frame
            assert c.sample_window()["next"] == dict(total=S, first=0, divisor=S, accumulate=0, advance=0), c.sample_window()
            self.same_clamp(c, None, "a clone")  # the clamp is per scene and off by default, whatever the parent's (which apply() compares)
            self.same_bound(c, self.shape, "the clone's clip bound")
            mine = np.ones((sc.height, sc.width), bool)
            if subset:
                mine[:R.TILE, :R.TILE] = False  # tile 0 is not the clone's
            # (the default window on the wavefront pipeline: under a layout the clone's frame is settled like the scene's own)
            self.on_device(c, [np.where(mine, x, 0).astype(np.uint16) for x in self.lw.planes(self.described_pose, self.shape)],
                           settles((S, 0, S, 0, 0), R.PIPELINE_WAVEFRONT), "of the clone's frame",
                           tiles=len(tiles) if subset else None)
            if subset:
                refusal(c.temporal, "every tile of the image", "temporal on a tile subset")
        finally:
            c.close()


    # -- scene edits: the look changes in place; buffers, window, history, mark and group table stay, which the later steps prove
    def rows(self):
        return np.asarray(self.rs.scene_view("tri_shade")).reshape(-1, 24).view(np.int32).copy()

    def same_class(self, look, what):
        want = R.path_class(world(self.w.name, look).base)
        assert want == look_class(self.name, look)
        assert self.rs.path_class() == want, f"{what}: the scene's path class is {self.rs.path_class()}, the model's {want}"

    def do_lights(self, name):
        if self.rs:
            new = self.after(("lights", name))
            arrays = look_parts(self.name)["lights"][name]
            self.rs.set_lights(arrays)
            self.same_class(new, f"after set_lights({name})")
            for k in R.LIGHT_FIELDS:
                assert np.asarray(getattr(self.rs.scene, k)).tobytes() == np.ascontiguousarray(arrays[k]).tobytes(), \
                    f"after set_lights({name}): the scene's description differs in {k}"

    def do_materials(self, arg):
        if self.rs:
            name, ids = arg
            new = self.after(("materials", arg))
            self.rs.set_materials(look_parts(self.name)["materials"][name], None if ids is None else look_ids(self.name, ids))
            self.staged |= ids is not None
            self.same_class(new, f"after set_materials({name}, {ids})")
            count = look_parts(self.name)["counts"][name]
            assert self.rs.scene.material_count == count, f"after set_materials({name}): {self.rs.scene.material_count} materials, the model has {count}"
            differs(self.rows()[:, 21], look_ids(self.name, new[2]), f"word 21 of the shading rows after set_materials({name}, {ids})")

    def do_ids(self, arg):
        if self.rs:
            ids, form = arg
            want = look_ids(self.name, ids)
            before = self.rows()
            if form == "torch":
                import torch
                self.rs.set_materials(tri_material=torch.from_numpy(want).to(torch.device("cuda", 0)))
            else:
                self.rs.set_materials(tri_material=want)
                self.staged = True
            self.same_class(self.after(("ids", arg)), f"after the ids {ids}")
            now = self.rows()
            differs(now[:, 21], want, f"word 21 of the shading rows after the ids {ids} ({form})")
            differs(np.delete(now, 21, axis=1), np.delete(before, 21, axis=1), f"the other 23 words of the shading rows after the ids {ids}")
            row = np.asarray(self.rs.scene_view("tri_shade_row")).reshape(-1, 32).view(np.uint32)
            rec = np.asarray(self.rs.scene_view("tri_rec")).reshape(-1, 16).view(np.uint32)
            differs(row[:, 24:28], rec[:, 0:4], f"words 24..27 of the shading rows (vertex a) after the ids {ids}")

    def do_refused_edit(self, variant):
        """One illegal argument: the code and the text, and addresses and byte count as they were -- but for the staging of host
        ids, which the header gives to the first call that brings some, refused or not: ids are checked on the device."""
        if not self.rs:
            return
        rs, lib, parts = self.rs, R.lib(), look_parts(self.name)
        pointers, held = rs.pointers(), rs.bytes()
        ids = look_ids(self.name, self.look[2])
        mats = {k: np.ascontiguousarray(v) for k, v in parts["materials"][self.look[1]].items()}
        count, T = parts["counts"][self.look[1]], ids.shape[0]
        L = {k: np.ascontiguousarray(v) for k, v in parts["lights"]["sun_spot"].items()}
        p = {k: R._ptr(v) for k, v in L.items()}
        size, start, tex = mats["mat_size"].reshape(-1, 2), mats["mat_start"].reshape(-1), mats["textures"].reshape(-1, 4)
        code, grown = -1, 0
        if variant == "shrink":  # tables of max_id materials, without ids: the resident max_id is out of range
            m = self.max_id()
            assert 1 <= m < count
            rc, code, text = rs.try_set_materials(dict(mat_size=size[:5 * m].copy(), mat_start=start[:5 * m + 1].copy(), textures=tex)), -5, REJECTED
        elif variant in ("bad_first", "bad_last"):
            bad = ids.copy()
            bad[0 if variant == "bad_first" else T - 1] = count
            rc, code, text = rs.try_set_materials(tri_material=bad), -5, REJECTED
            grown, self.staged = (0 if self.staged else 4 * T), True
        elif variant == "host_pointer":
            rc = lib.rtHipSceneSetMaterials(rs.handle, ctypes.byref(R.MaterialUpdate(0, 0, None, None, 0, None, R._ptr(ids), 1)))
            text = "not device memory"
        elif variant == "neither":
            rc, text = lib.rtHipSceneSetMaterials(rs.handle, ctypes.byref(R.MaterialUpdate())), "neither"
        elif variant == "past_atlas":
            past = start.copy()
            ch = int(np.flatnonzero(size[:, 0] > 0)[0])  # the first channel that holds texels, moved one texel past the atlas
            past[ch] = len(tex) - int(size[ch, 0]) * int(size[ch, 1]) + 1
            rc = lib.rtHipSceneSetMaterials(rs.handle, ctypes.byref(R.MaterialUpdate(1, count, R._ptr(size), R._ptr(past), len(tex), R._ptr(tex), None, 0)))
            text = "exceed"
        elif variant == "65536_lights":
            rc, text = lib.rtHipSceneSetLights(rs.handle, ctypes.byref(R.Lights(65536, *[p[k] for k in R.LIGHT_FIELDS]))), "too large"
        else:
            rc = lib.rtHipSceneSetLights(rs.handle, ctypes.byref(R.Lights(2, p["light_type"], None, p["light_dir"], p["light_col"], p["light_radius"],
                                                                          p["light_half_att"])))
            text = "null light array"
        assert int(rc) == code and text in R.last_error(), f"refused edit ({variant}): returned {rc} with {R.last_error()!r}, expected {code} with {text!r}"
        if code == -5:
            assert "scene rejected" in R.last_error(), R.last_error()
        assert rs.pointers() == pointers, f"refused edit ({variant}): the scene's addresses changed"
        assert rs.bytes() - held == grown, \
            f"refused edit ({variant}): the scene holds {rs.bytes()} bytes, {held} before it (staging expected: exactly {grown})"

    # -- mattes: the group table is state; a call reads the last frame's window for its defaults and leaves window and buffers alone
    def do_matte_groups(self, seed=None):
        if self.rs:
            self.rs.set_matte_groups(None if seed is None else group_table(self.w.base.triangle_count, seed))

    def matte_table(self, kind):
        if kind == "triangle":
            return None
        return MA.material_table(look_ids(self.name, self.look[2])) if kind == "material" else group_table(self.w.base.triangle_count, self.groups)

    def do_mattes(self, arg):
        kind, n, layers, window = arg
        S = self.samples
        last = (S, 0) if self.window_last is None else self.window_last[:2]
        defaults = dict(kind="triangle", select=(), layers=4, total=last[0], first=last[1], samples=S)
        if self.rs:
            got = self.rs.matte_defaults()
            assert got == defaults, f"the matte defaults are {got}, the model's last frame gives {defaults}"
        if self.refuses(("mattes", arg)):
            if self.rs:
                refusal(lambda: self.rs.mattes(kind="group", layers=layers), "group table", "kind GROUP without a table")
            return
        N, f, C_ = window or (last[0], last[1], S)
        ids = self.w.sample_ids(self.pose, self.shape, N, f, C_)
        table = self.matte_table(kind)
        select = selection(MA.table_ids(ids, table), n)
        want = MA.mattes(ids, table, select, layers, C_, shape=(self.w.height, self.w.width))
        self.notes.append(("mattes", dict(kind=kind, window=(N, f, C_), layers=layers, select=select), want))
        if self.rs:
            kw = {} if window is None else dict(total=N, first=f, samples=C_)
            got = self.rs.mattes(kind=kind, select=select, layers=layers, **kw)
            assert sorted(got) == sorted(k for k in ("select", "layer_id", "layer_coverage", "rest") if k != "select" or select), sorted(got)
            for k in got:
                differs(got[k], want[k], f"matte output {k} ({kind}, select {select}, K = {layers}, window {(N, f, C_)}) at {self.here()}")


def describe(steps):
    return "; ".join(f"{i}: {k}" + ("" if a is None else f"({a})") for i, (k, a) in enumerate(steps))


def play(name, seed, part, last=None, report=None, layout=None, tally=None):
    """Plays one sequence on the device and stops at the first mismatch: one pass, nothing is tried again.  The scene is always closed
    (twins and clones close themselves).  report(step number, step, verdict) is called after every step.
    layout (a key of LAYOUTS): its variables stand in os.environ from before the scene is created -- so the clones and twins made on
    the way are laid out like it -- until the sequence is over, when the values of before are put back and the library's tuning
    values are set from them, so the next scene anyone creates is on the defaults again; frames that settle are rendered
    SETTLED_FRAMES times (Session.on_device), and `tally` (a Counter) takes what their last repeats reported."""
    seq = part_of(name, seed, part)
    steps = seq["steps"] if last is None else seq["steps"][:last + 1]
    w = world(name)
    under = f" under the layout {layout}" if layout else ""
    env = LAYOUTS[layout] if layout else {}
    before = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        rs = R.ResidentScene(w.state(*seq["start"]), 0)
        try:
            s = Session(w, seq["start"], rs, edit=is_edit(name, seed), post=is_post(name, seed), layout=layout, tally=tally)
            s.same_window("a fresh scene")
            s.same_clamp(rs, None, "a fresh scene")
            for i, step in enumerate(steps):
                try:
                    s.apply(step)
                except (AssertionError, RuntimeError) as e:
                    if report:
                        report(i, step, f"MISMATCH: {e}")
                    raise AssertionError(f"{name} seed {seed} part {part}{under}, step {i} {step}: {e}\nstarted at {seq['start']}; steps so far: "
                                         f"{describe(steps[:i + 1])}") from e
                if report:
                    report(i, step, "ok")
        finally:
            rs.close()
    finally:
        for k, v in before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        if env:
            R.apply_env_tuning()
    return len(steps)
