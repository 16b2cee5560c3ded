"""NumPy / torch restatement of the tail of the reference's production path, the checker of ``utils.pxd_digits`` (tests only).

Restates ``Physics_Analysis/create_g1.py:69-79`` (paths relative to the reference's repository root) on a batch of sensor images that is
already in detector units and cropped, ``[N, H, W]`` -- what ``:69-75`` (threshold, ``256^x - 1``, crop) leave before ``.to(uint8)``:
* ``:73``  ``.clamp_(0, 255).to(torch.uint8)``: truncation to the uint8 charge (NaN, which the reference never meets, counts as 0);
* ``:77``  ``imgs.nonzero(as_tuple=True)``: the digits, in row-major order = ascending flat index;
* ``:79``  ``imgs[nonzeros]``: their charges.
One extension, off at ``threshold = 0`` (the reference's production behaviour): a pixel below ``threshold`` is no digit
(``Evaluation/eval_all.py:115``, ``imgs[imgs < THRESHOLD] = 0``, applied to the value before truncation).
"""
import numpy as np
import torch


def digits(images, threshold=0.0):
    """``(index int32 [total], charge uint8 [total], counts int32 [N], total)`` of ``images`` ``[N, H, W]`` (fp32 or uint8, array or
    tensor on the host)."""
    t = torch.as_tensor(np.asarray(images))
    N, H, W = t.shape
    if t.dtype == torch.uint8:
        q = t.clone()
    else:
        q = torch.nan_to_num(t.float(), nan=0.0).clamp_(0, 255).to(torch.uint8)       # create_g1.py:73
    q[~(t.float() >= threshold)] = 0                                                   # eval_all.py:115 (no-op at threshold 0)
    nonzeros = q.nonzero(as_tuple=True)                                                # create_g1.py:77
    charges = q[nonzeros]                                                              # :79
    n, r, c = nonzeros
    index = (n * (H * W) + r * W + c).to(torch.int32)
    counts = torch.bincount(n, minlength=N).to(torch.int32)
    return index, charges, counts, int(index.numel())


def queue_format(images, threshold=0.0):
    """What ``create_g1.generate`` returns (:79): ``((idx, ucell, vcell) lists, charges list)``."""
    t = torch.as_tensor(np.asarray(images))
    index, charges, _, _ = digits(t, threshold)
    N, H, W = t.shape
    index = index.to(torch.int64)
    return ((index // (H * W)).tolist(), (index % (H * W) // W).tolist(), (index % W).tolist()), charges.tolist()
