"""``vmas_world_step_env_checked`` without a GPU: the symbol is exported and declared (header, ``_abi.EXPORTED_SYMBOLS``), and
what it refuses comes back as -1 + a message, in front of any launch - on a planning world (device -1), which has no device side."""
import ctypes as C
import os
import re

import pytest

from vectorizedmultiagentsimulator_amd import _abi as A

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


@pytest.fixture(scope="module")
def lib():
    return A.load_library()


def test_the_entry_is_exported_and_declared(lib):
    assert "vmas_world_step_env_checked" in A.EXPORTED_SYMBOLS
    assert hasattr(lib, "vmas_world_step_env_checked")
    assert lib.vmas_world_step_env_checked.restype is C.c_int and len(lib.vmas_world_step_env_checked.argtypes) == 13
    header = open(os.path.join(ROOT, "include", "vmas_env_hip.h")).read()
    decl = re.search(r"int vmas_world_step_env_checked\(([^;]*)\);", header)
    assert decl is not None, "declared in include/vmas_env_hip.h"
    assert len(decl.group(1).split(",")) == 13, "the ctypes prototype follows the header"


def test_the_entry_refuses_with_a_message(lib):
    from vectorizedmultiagentsimulator_amd.scenarios.balance import Scenario

    fn = lib.vmas_world_step_env_checked
    ing = A.IngestArgs()
    word = (C.c_uint32 * 16)()  # stands for the flag block: never read by a call that is refused
    wp = C.cast(word, C.c_void_p)
    assert fn(None, None, None, 64, None, C.byref(ing), wp, wp, A.POST_BALANCE, None, None, 1, None) == -1
    assert b"null world" in lib.vmas_last_error()
    world = Scenario().env_make_world(4, "cpu", n_agents=3)
    cd = world.spec.to_ctypes()
    h = C.c_void_p()
    assert lib.vmas_world_create(C.byref(cd.world), 4, -1, C.byref(h)) == 0, A.last_error()
    try:
        assert fn(h, None, None, 64, None, C.byref(ing), None, wp, A.POST_BALANCE, None, None, 1, None) == -1
        assert b"flag word" in lib.vmas_last_error()
        assert fn(h, None, None, 64, None, C.byref(ing), wp, None, A.POST_BALANCE, None, None, 1, None) == -1
        assert b"flag word" in lib.vmas_last_error()
        for n in (0, 2, -1):
            assert fn(h, None, None, 64, None, C.byref(ing), wp, wp, A.POST_BALANCE, None, None, n, None) == -1
            assert b"single steps only" in lib.vmas_last_error()
        assert fn(h, None, None, 64, None, None, wp, wp, A.POST_BALANCE, None, None, 1, None) == -1
        assert b"ingest" in lib.vmas_last_error()
        assert fn(h, None, None, 64, None, C.byref(ing), wp, wp, A.POST_BALANCE, None, None, 1, None) == -1
        assert b"planning world" in lib.vmas_last_error()
        assert all(x == 0 for x in word), "a refused call advances no sequence number"
    finally:
        lib.vmas_world_destroy(h)
