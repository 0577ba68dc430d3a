"""Records tests/golden/uperhead_fwd.npz: inputs, a state dict and the train-mode and eval-mode forward outputs of the
reference's own ``UPerHead`` (models/decoders/UPernet.py of the reference checkout given on the command line), on the
CPU in fp32.  Data only: tests/test_uper_host.py loads the file and checks that tests/uper_ref.py reproduces both
outputs.  Never imported by a test.

    python tests/golden/make_uper_golden.py /path/to/reference
"""
import importlib.util
import os
import sys

import numpy as np
import torch

IN_CHANNELS, CHANNELS, NUM_CLASSES, B = [8, 16, 24, 32], 16, 5, 2
GRIDS = [(12, 10), (6, 5), (3, 3), (2, 2)]


def main(reference):
    spec = importlib.util.spec_from_file_location("ref_upernet", os.path.join(reference, "models", "decoders", "UPernet.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.manual_seed(20)
    head = mod.UPerHead(in_channels=IN_CHANNELS, num_classes=NUM_CLASSES, channels=CHANNELS)
    g = torch.Generator().manual_seed(21)
    with torch.no_grad():
        for m in head.modules():            # non-trivial BatchNorm parameters and running statistics
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.add_(0.1 * torch.randn(m.weight.shape, generator=g))
                m.bias.add_(0.1 * torch.randn(m.bias.shape, generator=g))
                m.running_mean.copy_(torch.rand(m.running_mean.shape, generator=g) * 0.2 - 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
    feats = [torch.randn(B, c, h, w, generator=g) for c, (h, w) in zip(IN_CHANNELS, GRIDS)]
    out = {f"feat{i}": f.numpy() for i, f in enumerate(feats)}
    out.update({"sd." + k: v.clone().numpy() for k, v in head.state_dict().items()})   # before the train-mode run
    with torch.no_grad():
        out["out_eval"] = head.eval()([f.clone() for f in feats]).numpy()
        out["out_train"] = head.train()([f.clone() for f in feats]).numpy()
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "uperhead_fwd.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
