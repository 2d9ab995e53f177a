"""``World.step`` on the autograd tape: the forward is the HIP step kernel, the backward ONE launch of the backward
kernel (csrc/vmas_vjp.hip through ``HipWorld.step_vjp``) - no chain of small tensor ops, no tape of them.

Served: sphere-only worlds (``HipWorld.vjp_supported()``; DESIGN.md "Backward of World.step").  First order only: the
backward is ``once_differentiable``.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable


class _WorldStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hw, exact, state, agent_ft):
        # the inputs stay as they are (they are what the backward re-runs the step from); clones are stepped in place
        out_state = state.clone(memory_format=torch.contiguous_format)
        out_ft = agent_ft.clone(memory_format=torch.contiguous_format)
        hw.step(state=out_state, agent_ft=out_ft, exact=exact)
        ctx.hw = hw
        ctx.save_for_backward(state, agent_ft)
        return out_state, out_ft

    @staticmethod
    @once_differentiable
    def backward(ctx, g_state, g_ft):
        state, agent_ft = ctx.saved_tensors
        g_state_in, g_ft_in = ctx.hw.step_vjp(state.contiguous(), agent_ft.contiguous(), g_state, g_ft)
        return None, None, g_state_in, g_ft_in


def world_step(hw, state: torch.Tensor, agent_ft: torch.Tensor, exact: bool = False):
    """One ``World.step()`` of ``hw`` (a ``HipWorld``) from the packed ``state`` [E, 6, ld] / ``agent_ft`` [A, 3, ld] ->
    ``(state', agent_ft')``, fresh tensors that autograd differentiates with respect to both inputs.  ``agent_ft'`` is
    the force buffer as the step leaves it (clamped where agents have max_f / f_range / max_t / t_range).  ``exact``:
    as ``HipWorld.step`` (for the worlds served here - sphere-sphere pairs only - it changes nothing: such a pair's force
    is exactly 0 wherever the bounding circles do not overlap)."""
    why = hw.vjp_supported()
    if why is not None:
        raise NotImplementedError(why)
    return _WorldStep.apply(hw, bool(exact), state, agent_ft)
