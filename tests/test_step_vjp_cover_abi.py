"""Worlds (g), (h), (i) of test_step_vjp_cover_gpu.py without a GPU: the backward kernel's planner serves them, every
designated environment is in its regime and no other (counted from the float64 restatement), the recorded seed is the first
whose float64 branch margins are all >= 1e-4, and the float32 restatement's own forward error leaves the kernel three
quarters of the forward check's 1e-5 (figures: DESIGN.md 3.4b)."""
import pytest
import torch

from test_step_vjp_cover_gpu import CASES, CHAIN, SEEDS, build_world, chained, check_world, forward_error
from test_step_vjp_shapes_gpu import restate
from vectorizedmultiagentsimulator_amd.differentiable import planning_refusal


@pytest.mark.parametrize("name", list(SEEDS))
def test_the_planner_serves_the_world(name):
    assert planning_refusal(build_world(name, 8).spec) is None


@pytest.mark.parametrize("name,batch", CASES)
def test_every_designated_environment_is_in_its_regime_clear_of_every_kink(name, batch):
    margins = []
    spec, state, ft, out64 = check_world(name, batch, margins=margins)  # (asserts the coverage)
    assert min(margins) >= 1e-4, f"a branch quantity is within 1e-4 of its kink: {min(margins):.2e}"
    with torch.no_grad():
        share = forward_error(restate(spec, state.to(torch.float32), ft.to(torch.float32)), out64)
    print(f"{name}/{batch}: smallest margin {min(margins):.2e}, float32 restatement's forward error {share:.3f} of the check's 1e-5")
    assert share <= 0.25


@pytest.mark.parametrize("name,batch", CASES)
def test_the_recorded_seed_is_the_first_clear_of_every_kink(name, batch):
    for seed in range(SEEDS[name][batch]):
        margins = []
        check_world(name, batch, seed, margins)
        assert min(margins) < 1e-4, seed


def test_the_chained_steps_stay_clear_of_every_kink_from_the_first_such_seed():
    for seed in range(CHAIN[2] + 1):
        margins, (*_, leaves, chain) = [], chained(seed)
        with torch.no_grad():
            chain(margins, *leaves)
        assert (min(margins) >= 1e-4) == (seed == CHAIN[2]), (seed, min(margins))
