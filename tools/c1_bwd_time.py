"""Backward of a 1x1x1 convolution + BatchNorm at the batch-4 layer shapes, split route against the fused launch
(csrc/conv1_bwd_fused.hip), under HIP events:
    python tools/c1_bwd_time.py [reps]
Both routes are driven through ops.convbn3d's autograd nodes, so both include the BatchNorm's reduce + finalize passes;
those are timed alone as well and subtracted ("after reduce"), which is what the fused launch replaces.  GB/s are against
the bytes the fused form has to move: T = one pass over a 32-channel tensor, 4T for one input (read dz, y, x; write dx),
6T for two (read dz, y, x, x2; write dx, dx2)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dcanet_amd  # noqa: F401,E402
from dcanet_amd import ops  # noqa: E402

DEV = "cuda"
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10


def timed(fn, reps=REPS):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3      # us


def case(name, dims, two, slope):
    N, C = 4, 32
    x = torch.randn((N, C) + dims, device=DEV).requires_grad_()
    x2 = torch.randn((N, C) + dims, device=DEV).requires_grad_() if two else None
    conv = torch.nn.Conv3d(C * (2 if two else 1), C, 1, bias=False).to(DEV)
    bn = torch.nn.BatchNorm3d(C).to(DEV).train()
    gz = torch.randn((N, C) + dims, device=DEV)
    S = dims[0] * dims[1] * dims[2]
    T = N * C * S * 4
    out = {}
    for route, on in (("split", False), ("fused", True)):
        ops.C1_BWD_FUSE = on
        z = ops.convbn3d(x, conv, bn, slope, x2=x2)
        wrt = [x] + ([x2] if two else []) + [conv.weight, bn.weight, bn.bias]
        out[route] = timed(lambda: torch.autograd.grad(z, wrt, gz, retain_graph=True))
        del z
    # the reduce + finalize passes alone (common to both routes)
    y = torch.randn((N, C) + dims, device=DEV)
    stats = torch.cat([torch.zeros(C), torch.ones(C), torch.ones(C), torch.zeros(C)]).to(DEV)
    lib = ops._L()
    part = torch.empty((C * lib.dca_bn_num_chunks(C, S) * 2,), device=DEV, dtype=torch.float64)
    dgb = torch.empty((4 * C,), device=DEV)
    red = timed(lambda: ops._chk(lib.dca_bn_backward_reduce(ops._ptr(gz), ops._ptr(y), ops._ptr(stats), ops._ptr(part),
                                                           ops._ptr(dgb), N, C, S, float(slope), 1, ops._stream()), "reduce"))
    passes = 6 if two else 4
    gb = passes * T / 1e9
    s, f = out["split"] - red, out["fused"] - red
    print("%-34s reduce %7.1f us | after reduce: split %7.1f us, fused %7.1f us (%dT = %.2f GB -> %.2f TB/s), saved %6.1f us"
          % (name, red, s, f, passes, gb, gb / (f * 1e-6) / 1e3, s - f))


if __name__ == "__main__":
    case("redir 32->32 4x32x48x136x240", (48, 136, 240), False, 1.0)
    case("fuse (32+32)->32 4x32x48x136x240", (48, 136, 240), True, 1.0)
    case("proj 32->32 4x32x24x68x120", (24, 68, 120), False, 0.1)
