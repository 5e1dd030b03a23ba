"""CPU restatements for tests/test_evaluate.py.  resize_fixation is the reference's avsp_dataloader.py:16-31 without its
Python loop; tools/gen_eval_golden.py asserts it against the reference's own function on every fixture case.
resize_bilinear is the yardstick of mspi_amd.evaluate.resize_maps.  Neither is imported by mspi_amd."""
import numpy as np
import torch


def resize_fixation(image, row, col):
    """float64 [row, col], as the reference returns: np.rint on the float64 products (np.round is half to even), the
    `== row` / `== col` step back as a minimum, one fancy-index assignment for all fixations."""
    image = np.asarray(image)
    out = np.zeros((row, col))
    ratio_row = row / image.shape[0]
    ratio_col = col / image.shape[1]
    coords = np.argwhere(image)
    r = np.minimum(np.rint(coords[:, 0] * ratio_row).astype(np.int64), row - 1)
    c = np.minimum(np.rint(coords[:, 1] * ratio_col).astype(np.int64), col - 1)
    out[r, c] = 1
    return out


def resize_bilinear(x, size):
    """float64 [B, Ho, Wo] from [B, H, W] (uint8 or float): torch's bilinear interpolation with align_corners=False in
    float64 on the CPU -- the pixel-centre convention of cv2.INTER_LINEAR, src = (dst + 0.5) * in / out - 0.5 with clamped
    edges and no antialiasing.  OpenCV is not available where these tests run, so parity with cv2.resize itself (its
    fixed-point path for uint8 in particular) stays unpinned, as for oracle.restate.postprocess_u8."""
    x = torch.as_tensor(x).double()[:, None]
    return torch.nn.functional.interpolate(x, size=tuple(size), mode="bilinear", align_corners=False)[:, 0]
