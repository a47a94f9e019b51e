"""Generates tests/golden/torch_graph_golden.npz: the REFERENCE's fp32 graph ``DMCI.forward_one_frame(x, 20,
recon_only=True)`` (/root/reference/src/models/image_model.py:150-192) with the seeded synthetic weights on a seeded
1x3x64x128 picture, stored in fp32 - what tests/test_oracle_cpu.py::test_torch_restatement_of_the_reference_cpu_path
holds oracle/torch_graph.py to (run in the build container, where /root/reference exists).

Usage: python tests/golden/make_torch_graph_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from dcvc_amd import arch, synthetic  # noqa: E402
from oracle import build_oracle, rans as orc  # noqa: E402

QP = 20


def main():
    build_oracle.build_ref()
    sys.modules["MLCodec_extensions_cpp"] = orc.load_ref()
    sys.path.insert(0, "/root/reference")
    from src.models.image_model import DMCI
    net = DMCI().eval()
    net.load_state_dict(synthetic.synthetic_state_dict(arch.dmci_spec(), 0), strict=True)
    x = torch.rand((1, 3, 64, 128), generator=torch.Generator().manual_seed(3)) - 0.5
    with torch.no_grad():
        x_hat = net.forward_one_frame(x, torch.tensor([QP]), recon_only=True)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "torch_graph_golden.npz"),
                        x=x.numpy(), x_hat=x_hat.numpy(), qp=np.array([QP]))
    print("wrote torch_graph_golden.npz, x_hat std %.4f" % x_hat.std().item())


if __name__ == "__main__":
    main()
