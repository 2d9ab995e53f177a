"""The planner of the LIDAR's backward kernel (vmas_world_cast_rays_vjp_check) on a planning world: no GPU."""
import ctypes as C

from vectorizedmultiagentsimulator_amd import _abi as A
from vectorizedmultiagentsimulator_amd.scenarios.navigation import Scenario


def test_navigation_is_served_and_a_world_without_sensors_says_so():
    lib, h = A.load_library(), C.c_void_p()
    desc = Scenario().env_make_world(4, "cpu", n_agents=8).spec.to_ctypes()
    assert len(desc.spec.lidars) == 8 and desc.max_rays == 12
    assert lib.vmas_world_create(C.byref(desc.world), 1, -1, C.byref(h)) == 0, A.last_error()
    assert lib.vmas_world_cast_rays_vjp_check(h) == -1 and "no sensors registered" in A.last_error()
    assert lib.vmas_world_set_lidars(h, desc.lidars, 8) == 0, A.last_error()
    runs, units, waves, lds = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
    assert lib.vmas_world_cast_rays_vjp_check(h) == 0, A.last_error()
    assert lib.vmas_world_cast_rays_vjp_plan(h, C.byref(runs), C.byref(units), C.byref(waves), C.byref(lds)) == 0
    # 8 agents x (x, y, rotation) staged and carried, 8 units of 3 carrier rows + 2 per sphere target, 256 B a row
    assert (runs.value, units.value, waves.value, lds.value) == (1, 8, 8, 256 * (8 * 6 + 8 * (3 + 2 * 7)))
    # everything that touches the device still fails on a planning world
    assert lib.vmas_world_cast_rays(h, C.c_void_p(64), 64, C.c_void_p(64), None) == -1 and "planning world" in A.last_error()
    assert lib.vmas_world_cast_rays_vjp(h, C.c_void_p(64), 64, C.c_void_p(64), C.c_void_p(64), None) == -1
    assert "planning world" in A.last_error()
    lib.vmas_world_destroy(h)
