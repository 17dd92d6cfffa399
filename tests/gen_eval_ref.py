"""Float64 host restatement of the reference's generation-quality evaluation (evaluation/generation_eval_sagittal.py and
generation_eval_coronal.py: calculate_iou :11-17, calculate_dice :19-28, relative_volume_difference :31-37, process_images :39-103, the
skip and average rule of main() :140-158), shared by tools/make_golden_gen_eval.py (as the stand-in for scikit-image's metrics) and the GPU
tests (as the host side of every comparison).

psnr / ssim restate scikit-image 0.22's peak_signal_noise_ratio and structural_similarity for two float64 2-D images with an explicit
data_range: 7x7 uniform window (scipy.ndimage.uniform_filter, as scikit-image uses), sample covariance 49/48, K1 0.01, K2 0.03, 3-pixel
border cropped, float64 mean.  scikit-image is not installed here, so these two are pinned against their published definition only (like
oracle/restate.eval_ssim, f3); everything else -- masks, counts, slice range and selection, crop rows, data ranges, NaN handling, averages --
is the reference's own decision, recorded in fixture G14.
"""
import math
import warnings

import numpy as np
from scipy.ndimage import uniform_filter

VIEW_AXIS = {'sagittal': 2, 'coronal': 1}


def psnr(a, b, data_range):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        raise ValueError('Input images must have the same dimensions.')
    err = np.mean((a - b) ** 2, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return float(10 * np.log10((float(data_range) ** 2) / err))


def ssim(a, b, data_range):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        raise ValueError('Input images must have the same dimensions.')
    if np.any((np.asarray(a.shape) - 7) < 0):
        raise ValueError('win_size exceeds image extent.')
    R = float(data_range)
    ux, uy = uniform_filter(a, size=7), uniform_filter(b, size=7)
    uxx, uyy, uxy = uniform_filter(a * a, size=7), uniform_filter(b * b, size=7), uniform_filter(a * b, size=7)
    cov = 49.0 / 48.0
    vx, vy, vxy = cov * (uxx - ux * ux), cov * (uyy - uy * uy), cov * (uxy - ux * uy)
    C1, C2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    A1, A2, B1, B2 = 2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2
    with np.errstate(divide='ignore', invalid='ignore'):
        S = (A1 * A2) / (B1 * B2)
    return float(S[3:-3, 3:-3].mean(dtype=np.float64))


def calculate_iou(ori, fake):
    inter = np.sum(ori * fake)
    union = np.sum(ori + fake > 0)
    return 0 if union == 0 else inter / union


def calculate_dice(ori, fake):
    inter = np.sum(ori * fake)
    union = np.sum(ori) + np.sum(fake)
    return 0 if union == 0 else 2.0 * inter / union


def relative_volume_difference(ori, fake):
    vo, vf = np.sum(ori), np.sum(fake)
    return 0 if vo == 0 else np.abs(vo - vf) / vo


def _slice(vol, axis, z):
    return vol[:, :, z] if axis == 2 else vol[:, z, :]


def process_images(ori_ct, fake_ct, ori_seg, fake_seg, label, view='sagittal', record=None):
    """-> the seven values (global_psnr, global_ssim, patch_psnr, patch_ssim, iou, rv_diff, dice); `record` (a list) receives one dict per
    evaluated slice {z, x1, x2, R_patch, R_global, psnr_patch, ssim_patch, psnr_global, ssim_global}.  Raises ValueError like the reference."""
    ax = VIEW_AXIS[view]
    ori_ct, fake_ct = np.asarray(ori_ct, dtype=np.float64), np.asarray(fake_ct, dtype=np.float64)
    ori = (np.asarray(ori_seg, dtype=np.float64) == label).astype(np.float64)
    fake = (np.asarray(fake_seg, dtype=np.float64) == label).astype(np.float64)
    iou, dice, rvd = calculate_iou(ori, fake), calculate_dice(ori, fake), relative_volume_difference(ori, fake)
    loc = np.where(ori)[ax]
    if loc.size == 0:
        raise ValueError('min() arg is an empty sequence')
    z0, z1 = int(loc.min()), int(loc.max())
    n = z1 - z0 + 1
    m = int(n * 4 / 5)
    nz0 = z0 + (n - m) // 2
    lists = {k: [] for k in ('pp', 'ps', 'gp', 'gs')}
    recs = []
    for z in range(nz0, nz0 + m):
        o = _slice(ori, ax, z)
        if np.sum(o) > 400:
            rows = np.argwhere(o)[:, 0]
            x1, x2 = int(rows.min()), int(rows.max())
            a, b = _slice(ori_ct, ax, z), _slice(fake_ct, ax, z)
            ca, cb = a[x1:x2 + 1], b[x1:x2 + 1]
            Rp, Rg = float(ca.max() - ca.min()), float(a.max() - a.min())
            recs.append(dict(z=z, x1=x1, x2=x2, R_patch=Rp, R_global=Rg, psnr_patch=psnr(ca, cb, Rp), ssim_patch=ssim(ca, cb, Rp)))
    for r in recs:
        a, b = _slice(ori_ct, ax, r['z']), _slice(fake_ct, ax, r['z'])
        r['psnr_global'], r['ssim_global'] = psnr(a, b, r['R_global']), ssim(a, b, r['R_global'])
    for r in recs:
        for k, f in (('pp', 'psnr_patch'), ('ps', 'ssim_patch'), ('gp', 'psnr_global'), ('gs', 'ssim_global')):
            if not np.isnan(r[f]):
                lists[k].append(r[f])
    if record is not None:
        record.extend(recs)
    avg = {k: (float(np.mean(v)) if v else 0) for k, v in lists.items()}
    return avg['gp'], avg['gs'], avg['pp'], avg['ps'], float(iou), float(rvd), float(dice)


def main_average(results):
    """main()'s skip and average rule over a list of process_images results -> (dict of the seven np.mean values, kept count)."""
    keys = ('global_psnr', 'global_ssim', 'patch_psnr', 'patch_ssim', 'iou', 'rv_diff', 'dice')
    lists = {k: [] for k in keys}
    for r in results:
        if math.isnan(r[2]) or math.isnan(r[3]) or r[2] == 0 or r[3] == 0:
            continue
        for k, v in zip(keys, r):
            lists[k].append(v)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        return {k: float(np.mean(v)) for k, v in lists.items()}, len(lists['iou'])


def close(a, b, rtol=1e-9, atol=1e-12):
    """Equal NaN-ness and signed infinities, else |a - b| <= atol + rtol |b| (atol: SSIM means that are pure rounding noise around 0)."""
    a, b = float(a), float(b)
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    if math.isinf(a) or math.isinf(b):
        return a == b
    return abs(a - b) <= atol + rtol * abs(b)
