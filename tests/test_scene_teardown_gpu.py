"""A resident scene's teardown on the MI355X (run with -m gpu): a small mesh scene makes every store a scene makes on first use -- both
pass buffers, the denoiser's scratch, the query staging, the AO and bake scratch, the motion reference and staging, the temporal history
and moments, the camera move's sets and the geometry update's sets -- and is destroyed.  Three such lives in one process count the same
rtHipSceneBytes, and the device's free memory after the third destroy is not below that after the second (the first life is left out: it
warms state the runtime keeps)."""
import copy

import numpy as np
import pytest
import torch

import scenarios as SCN
from opencl_render_amd import raytrace as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu(hip_lib):
    if hip_lib.rtHipDeviceCount() < 1:
        pytest.fail("no HIP device: the teardown test cannot run (and the product has no CPU fallback)")


def one_life(sc):
    """bytes() of a scene that has made every lazily-made store; the scene is destroyed on return."""
    rs = R.ResidentScene(sc)
    try:
        rs.set_passes(alpha=True, depth=True, triangle=True, normal=True, albedo=True)
        rs.render()
        rs.sync()
        rs.finish()
        rs.denoise()
        rs.intersect(np.array([[0.25, 1.25, -2.0]] * 3, np.float32), np.array([[0, 0, 1], [0.1, -0.1, 1], [-0.1, 0.1, 1]], np.float32))
        rs.ambient_occlusion(rays=1)
        rs.bake_ambient_occlusion(4, 4, rays=1)
        rs.mark_motion()
        rs.motion()
        rs.temporal_variance(filter={})
        rs.look_at((0.3, 1.2, -2.0), (0.0, 0.75, 3.0), (0, 1, 0), np.radians(60.0))
        vertex = np.array(sc.vertex, np.float32)
        vertex[:, 0] += 0.0625
        rs.set_vertices(vertex, np.asarray(sc.tri_index))
        return rs.bytes()
    finally:
        rs.close()


def free_memory():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def test_three_lives_count_the_same_bytes_and_give_the_memory_back():
    sc = copy.copy(SCN.axis_sun_negative_zero_dir())  # 96 x 72: one tile
    sc.sample_count = 1
    assert R.tile_count(sc.width, sc.height) == 1
    counted, free = [], []
    for _ in range(3):
        counted.append(one_life(sc))
        free.append(free_memory())
    print(f"rtHipSceneBytes per life: {counted}; free device memory after each destroy: {free}")
    assert counted[0] > 0 and counted[1] == counted[0] and counted[2] == counted[0]
    assert free[2] >= free[1], f"free device memory fell by {free[1] - free[2]} bytes between the second and the third destroy"
