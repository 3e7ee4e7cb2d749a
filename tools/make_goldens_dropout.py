#!/usr/bin/env python3
"""Generate tests/golden/mlp_dropout.npz by running the REFERENCE's own Mlp (genie/st_transformer.py:7-25) in train mode.

Build-container only, like tools/make_goldens.py: /root/reference does not exist on the GPU box, so the arrays are committed and
this script documents how they were made.  Nothing of the reference's source is copied; only inputs and what it computed.

The module runs in float64 with mlp_drop = 0.25 on a (6, 8) input (hidden 32).  A forward hook on its one nn.Dropout, which the
forward calls twice (behind the GELU, behind fc2), records input and output of both calls; the keep masks are recovered as
"output != 0" (asserted: no input element is 0, and every kept element is input / (1 - p) to an ulp).  Stored: weights, input, both masks, p,
the output, a fixed cotangent, and the gradients of <output, cotangent> with respect to the input and the four parameters.
tests/test_train_dropout_cpu.py reproduces output and gradients with tests/dropout_model.mlp from the stored masks, which pins the
order (dropout behind the GELU and behind the bias of fc2) and the 1 / (1 - p) scaling to the reference itself.
"""
import os
import sys
import types

import numpy as np

os.environ["XFORMERS_DISABLED"] = "true"
import torch  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
OUT = os.path.join(REPO, "tests", "golden", "mlp_dropout.npz")
P, ROWS, D, RATIO = 0.25, 6, 8, 4.0


def main():
    def _no_xformers(*a, **k):
        raise RuntimeError("xformers is not available")
    ops = types.ModuleType("xformers.ops")
    ops.__dict__.update(LowerTriangularMask=object, memory_efficient_attention=_no_xformers, unbind=torch.unbind)
    xf = types.ModuleType("xformers")
    xf.ops = ops
    sys.modules.update({"xformers": xf, "xformers.ops": ops})   # imported by genie/attention.py:3; the Mlp never reaches it
    sys.path.insert(0, REF)
    from genie.st_transformer import Mlp

    torch.manual_seed(20240)
    mlp = Mlp(d_model=D, mlp_ratio=RATIO, mlp_bias=True, mlp_drop=P).double()
    with torch.no_grad():
        for prm in mlp.parameters():
            prm.copy_(torch.randn_like(prm) * 0.5)
    mlp.train()
    calls = []
    mlp.drop.register_forward_hook(lambda mod, inp, out: calls.append((inp[0].detach().clone(), out.detach().clone())))
    x = torch.randn(ROWS, D, dtype=torch.float64, requires_grad=True)
    cot = torch.randn(ROWS, D, dtype=torch.float64)
    with torch.enable_grad():
        y = mlp(x)
        (y * cot).sum().backward()
    assert len(calls) == 2, len(calls)
    masks = []
    for inp, out in calls:
        assert (inp != 0).all()
        keep = out != 0
        assert torch.allclose(out, torch.where(keep, inp / (1 - P), torch.zeros_like(inp)), rtol=1e-15, atol=0)
        assert 0 < int(keep.sum()) < keep.numel()
        masks.append(keep.numpy().astype(np.uint8))
    np.savez(OUT, p=np.float64(P), x=x.detach().numpy(), cot=cot.numpy(), m0=masks[0], m1=masks[1], y=y.detach().numpy(),
             fc1_w=mlp.fc1.weight.detach().numpy(), fc1_b=mlp.fc1.bias.detach().numpy(), fc2_w=mlp.fc2.weight.detach().numpy(),
             fc2_b=mlp.fc2.bias.detach().numpy(), dx=x.grad.numpy(), d_fc1_w=mlp.fc1.weight.grad.numpy(), d_fc1_b=mlp.fc1.bias.grad.numpy(),
             d_fc2_w=mlp.fc2.weight.grad.numpy(), d_fc2_b=mlp.fc2.bias.grad.numpy())
    print(OUT, os.path.getsize(OUT), "bytes; kept", [int(m.sum()) for m in masks], "of", [m.size for m in masks])


if __name__ == "__main__":
    main()
