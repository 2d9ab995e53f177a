"""CPU side of the backward of World.step: the C entries refuse bad arguments without touching a GPU, a planning world
tells whether the backward kernel serves it, and grad_enabled excludes the fused paths."""
import ctypes as C

import pytest

from vectorizedmultiagentsimulator_amd import _abi as A


def test_bad_arguments_are_refused_with_a_message_and_a_planning_world_reports_support():
    from golden_util import load
    from test_step_vjp_gpu import build_world

    lib = A.load_library()
    buf = C.c_void_p(64)  # never dereferenced: every check comes first, and a planning world never launches
    assert lib.vmas_world_step_vjp(None, buf, buf, 64, buf, None, buf, buf, None) == -1 and "null world" in A.last_error()
    assert lib.vmas_world_step_vjp_check(None) == -1 and "null world" in A.last_error()
    for spec, ok in ((build_world("b", 8).spec, True), (load("balance_n4").spec, False)):
        desc, h = spec.to_ctypes(), C.c_void_p()
        assert lib.vmas_world_create(C.byref(desc.world), 8, -1, C.byref(h)) == 0, A.last_error()
        assert (lib.vmas_world_step_vjp_check(h) == 0) == ok
        if ok:
            assert lib.vmas_world_step_vjp(h, buf, buf, 64, None, None, buf, buf, None) == -1 and "null buffer" in A.last_error()
            assert lib.vmas_world_step_vjp(h, buf, buf, 4, buf, None, buf, buf, None) == -1 and "ld" in A.last_error()
        else:
            assert "sphere-sphere" in A.last_error()
        lib.vmas_world_destroy(h)


def test_grad_enabled_excludes_the_fused_step():
    from vectorizedmultiagentsimulator_amd.environment import make_env

    with pytest.raises(AssertionError, match="grad_enabled"):
        make_env("navigation", num_envs=4, device="cpu", grad_enabled=True, fused=True)
