"""The stop rule of the adaptive entries (include/rt_capi.h, rt_accumulate_adaptive_device) in
numpy float64, one operation per line as the header writes it (numpy does not fuse), and the
frames the adaptive tests share."""
import numpy as np

W, H, AA = 24, 16, 8
# scene -> (width, height): 21x13 has ragged 8x8 tiles and list lengths that are no multiple of 64
FRAMES = {"c2": (24, 16), "c1": (24, 16), "glass": (21, 13), "mirror": (21, 13)}
RULE = dict(tolerance=0.05, lum_floor=0.01, min_samples=2)
SEED = 0x5EED


def converged(n, m1, m2, tolerance, lum_floor):
    """The rule's converged() for arrays of pixels; n >= 2.  False where a NaN appears."""
    with np.errstate(all="ignore"):
        nd = n.astype(np.float64)
        mean = m1 / nd
        prod = m1 * mean
        diff = m2 - prod
        var = diff / (nd - 1.0)
        err2 = var / nd
        ref = np.where(mean > lum_floor, mean, lum_floor)
        lim = tolerance * ref
        lim2 = lim * lim
        return err2 <= lim2


def stop_counts(per_sample_rgb, rule, sample_end, start=None):
    """The rule's loop on per_sample_rgb[s] = the [n,3] colours of sample s: (count int32 [n],
    sum float64 [n,3], moments float64 [n,2]).  start: a (count, sum, moments) to continue;
    None: the fresh state."""
    n_px = len(per_sample_rgb[0])
    if start is None:
        count = np.zeros(n_px, np.int32)
        total = np.zeros((n_px, 3), np.float64)
        moments = np.zeros((n_px, 2), np.float64)
    else:
        count, total, moments = (np.array(a, copy=True) for a in start)
    tol, floor, min_samples = rule["tolerance"], rule["lum_floor"], rule["min_samples"]
    per = np.stack([np.asarray(p, np.float64) for p in per_sample_rgb])  # [S, n, 3]
    for _ in range(sample_end):
        active = count < sample_end
        examined = active & (count >= min_samples)
        if examined.any():
            stop = np.zeros(n_px, bool)
            stop[examined] = converged(count[examined], moments[examined, 0],
                                       moments[examined, 1], tol, floor)
            active &= ~stop
        idx = np.flatnonzero(active)
        if not len(idx):
            break
        with np.errstate(all="ignore"):
            c = per[count[idx], idx]
            total[idx] = total[idx] + c
            lxy = c[:, 0] * 0.2126 + c[:, 1] * 0.7152
            lum = lxy + c[:, 2] * 0.0722
            moments[idx, 0] = moments[idx, 0] + lum
            moments[idx, 1] = moments[idx, 1] + lum * lum
        count[idx] = count[idx] + 1
    return count, total, moments
