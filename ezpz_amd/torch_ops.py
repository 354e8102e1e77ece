"""Solves inside a torch graph: `solve_params` is a differentiable batch solve with respect to the driven dimensions.

torch is imported here only (the package itself does not need it): `from ezpz_amd import torch_ops`.

    x = solve_params(system, x0, positions, params)      # [batch, n_vars], on params' device, on the current stream
    loss(x).backward()                                   # params.grad[b, j] = sum_i S[b, j, i] * grad_x[b, i]

Forward is `System.solve_batch_params_device`; backward evaluates `System.param_sensitivity_device` at the forward's answer
(S = -(JtJ + lam I)^-1 Jt dr/dp) and returns bmm(S, grad_x).  There is no gradient for x0: the answer of a
converged solve is a root of the constraints, which the start selects (which root, on a system that has several) but does not
move -- dx*/dx0 is zero wherever it exists; on an under-determined system the start does slide the answer along the free
directions, which this layer does not differentiate (it returns None for x0, like for every non-tensor argument).

`measure` reads reference dimensions back inside the graph:

    m = measure(system, x, records)                      # [..., n_meas] of x [..., n_vars], on the current stream
    measure(solve_params(system, x0, positions, params), records).sum().backward()   # fills params.grad

Forward is `System.measure_device`, backward `System.measure_vjp_device` (a per-variable sum in a fixed order: no atomics).
"""
import numpy as np
import torch

from .api import Config, stack_records
from ._lib import STATUS_DTYPE


class _SolveParams(torch.autograd.Function):
    @staticmethod
    def forward(ctx, system, x0, positions, params, config, lam):
        if not (x0.is_cuda and params.is_cuda) or x0.dtype != torch.float64 or params.dtype != torch.float64:
            raise ValueError("solve_params: x0 and params must be float64 tensors on the system's device")
        pos = np.ascontiguousarray(np.asarray(positions), dtype=np.uint32)
        x0c, pc = x0.detach().contiguous(), params.detach().contiguous()
        batch = x0c.shape[0]
        if x0c.shape != (batch, system.n_vars) or pc.shape != (batch, len(pos)):
            raise ValueError(f"solve_params: expected x0 ({batch}, {system.n_vars}) and params ({batch}, {len(pos)})")
        x = torch.empty_like(x0c)
        status = torch.zeros((batch, STATUS_DTYPE.itemsize), dtype=torch.uint8, device=x0c.device)
        stream = torch.cuda.current_stream(x0c.device).cuda_stream
        system.solve_batch_params_device(x0c.data_ptr(), pos, pc.data_ptr(), batch, x.data_ptr(), status.data_ptr(), stream=stream,
                                         config=config)
        ctx.system, ctx.pos, ctx.lam = system, pos, lam
        ctx.save_for_backward(x, pc)
        ctx.mark_non_differentiable(status)
        return x, status

    @staticmethod
    def backward(ctx, grad_x, _grad_status):
        x, pc = ctx.saved_tensors
        batch, k = pc.shape
        S = torch.empty((batch, k, ctx.system.n_vars), dtype=torch.float64, device=x.device)
        st = torch.empty(batch, dtype=torch.int32, device=x.device)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        ctx.system.param_sensitivity_device(x.data_ptr(), ctx.pos, pc.data_ptr(), batch, S.data_ptr(), st.data_ptr(), lam=ctx.lam,
                                            stream=stream)
        grad_params = torch.bmm(S, grad_x.contiguous().unsqueeze(2)).squeeze(2)
        return None, None, None, grad_params, None, None


class _Measure(torch.autograd.Function):
    @staticmethod
    def forward(ctx, system, x, records):
        if not x.is_cuda or x.dtype != torch.float64 or x.dim() < 1 or x.shape[-1] != system.n_vars:
            raise ValueError(f"measure: x must be a float64 tensor [..., {system.n_vars}] on the system's device")
        recs = stack_records(records)
        xc = x.detach().contiguous()
        lead = tuple(xc.shape[:-1])
        batch = int(np.prod(lead, dtype=np.int64))
        m = torch.zeros(lead + (len(recs),), dtype=torch.float64, device=xc.device)
        flags = torch.zeros(lead + (len(recs),), dtype=torch.uint8, device=xc.device)
        stream = torch.cuda.current_stream(xc.device).cuda_stream
        system.measure_device(xc.data_ptr(), recs, batch, m.data_ptr(), flags_ptr=flags.data_ptr(), stream=stream)
        ctx.system, ctx.recs, ctx.batch = system, recs, batch
        ctx.save_for_backward(xc)
        ctx.mark_non_differentiable(flags)
        return m, flags

    @staticmethod
    def backward(ctx, grad_m, _grad_flags):
        (xc,) = ctx.saved_tensors
        gm = grad_m.contiguous()
        gx = torch.zeros_like(xc)
        stream = torch.cuda.current_stream(xc.device).cuda_stream
        ctx.system.measure_vjp_device(xc.data_ptr(), ctx.recs, gm.data_ptr(), ctx.batch, gx.data_ptr(), stream=stream)
        return None, gx, None


def measure(system, x, records, return_flags=False):
    """m [..., n_meas] = the reference dimensions `records` of `system` at x [..., n_vars] (`System.measure_device` on the current
    stream); differentiable in x (`System.measure_vjp_device`), so measure(solve_params(system, x0, positions, params),
    records).sum().backward() fills params.grad.  return_flags: also the flags [..., n_meas] uint8."""
    m, flags = _Measure.apply(system, x, records)
    return (m, flags) if return_flags else m


def solve_params(system, x0, positions, params, config=None, lam=None, return_status=False):
    """x [batch, n_vars] = the solve of `system` from x0 with params [batch, len(positions)] overlaid; differentiable in params.
    return_status: also the solve's status records as a [batch, 32] uint8 tensor (view it with ezpz_amd._lib.STATUS_DTYPE)."""
    x, status = _SolveParams.apply(system, x0, positions, params, config or Config(), lam)
    return (x, status) if return_status else x
