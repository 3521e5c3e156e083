"""Wavefront pipeline modes (RT_WF_* tuning variables) that change only WHEN cells are visited and how rays are planned, cut and
batched, never the planes: shared by the parity tests (tests/test_parity_gpu.py) and the grid-walk edge tests
(tests/test_walk_edges_gpu.py)."""

MODES = [
    {"RT_WF_SEG": "16,16,16,16,16", "RT_WF_SEG_RAYS": "1,1,1,1"},   # every ray cut into segments of ~16 cell visits, whatever the round size
    {"RT_WF_SEG": "40,24,12,8,8"},                            # finer still for small rounds
    {"RT_WF_SEG": "4096,4096,4096,4096,4096"},                  # never cut
    {"RT_WF_APPEND_RAYS": "0"},                            # every round is an ordered one (planned by the logic kernel, counting sort)
    {"RT_WF_APPEND_RAYS": "4000000000", "RT_WF_ORDERED_FIRST": "0", "RT_WF_SEG": "24,24,24,24,24", "RT_WF_SEG_RAYS": "1,1,1,1"},  # no round is ordered: the trace kernel plans and cuts every ray
    {"RT_WF_ORDERED_FIRST": "0", "RT_WF_GROUP_RAYS": "16"},    # ... in workgroups of 16 rays
    {"RT_WF_LOOKAHEAD": "0"},                              # one ray in flight per path
    {"RT_WF_GROUPS": "3"},                                 # three concurrent tile groups per instance
    {"RT_WF_GROUPS": "2", "RT_WF_SEG": "16,16,16,16,16", "RT_WF_SEG_RAYS": "1,1,1,1", "RT_WF_LOOKAHEAD": "0"},
    {"RT_WF_SLICE_RAYS": "0"},                              # every round spreads its entries over all 256 queue slices per kind
    {"RT_WF_SLICE_RAYS": "4000000000", "RT_WF_SMALL_SLICES": "1", "RT_WF_APPEND_RAYS": "4000000000", "RT_WF_ORDERED_FIRST": "0"},  # one slice per kind from round 1 on, nothing ordered
    {"RT_WF_SLICE_RAYS": "20000", "RT_WF_SMALL_SLICES": "4", "RT_WF_APPEND_RAYS": "0", "RT_WF_SEG": "24,24,24,24,24", "RT_WF_SEG_RAYS": "1,1,1,1"},  # slices merge mid-frame, every round ordered and cut
    {"RT_WF_BLOCKING": "1"},                                # every batch of every frame watched
    {"RT_WF_FAST_QUOTIENT": "0"},                          # every wave divides the long way (the default picks per wave: test_kat_gpu.py)
]


def mode_id(env):
    return ",".join(f"{k[3:]}={v}" for k, v in env.items())
