"""An independent NumPy restatement of the SIFT keypoint detector pcc_sift_keypoints computes (PCL 1.7
SIFTKeypoint::detectKeypoints, reference src/comparator.cpp:435-469), for tests/test_sift_cpu.py and tools/exp_sift_ref.py.
Dense n x n matrices per octave, so for SMALL scenes only.

The run's dtype (float32 or float64) carries the intensities, the Gaussian weights, the sums, the responses and the DoG
columns; the sums are running sums over the row in INDEX order (one addition after the other, as PCL's loop adds, but not
in row order).  Everything that DECIDES which
entries take part is float32 in every run, so that all runs see the same rows: the octave clouds (voxel grid, sums in
float64 rounded once, as pcc_voxel_grid), the squared distances (FLANN's L2_Simple sum), the scales, sigma2, the radius
3 * scales[-1] and the 9 * sigma2 cut-offs, and the 25 nearest neighbours (ascending (d2, index))."""
import numpy as np

NEIGHBOURS = 25
MIN_POINTS = 25


def voxel_grid(points, words, leaf):
    """pcl::VoxelGrid with colour: (centroids float32 (m, 3), colour words (m,)) in ascending voxel index"""
    f32 = np.float32
    ok = np.isfinite(points).all(1)
    p, c = points[ok].astype(f32), words[ok].astype(np.uint32)
    if len(p) == 0:
        return p.reshape(0, 3), c
    inv = f32(1.0) / f32(leaf)
    mn = np.floor(p.min(0) * inv).astype(np.int64)
    mx = np.floor(p.max(0) * inv).astype(np.int64)
    dim = mx - mn + 1
    ijk = (np.floor(p * inv) - mn.astype(f32)).astype(np.int64)
    ijk = np.clip(ijk, 0, dim - 1)
    vid = (ijk[:, 2] * dim[1] + ijk[:, 1]) * dim[0] + ijk[:, 0]
    uniq, inverse, counts = np.unique(vid, return_inverse=True, return_counts=True)
    m = len(uniq)
    cen = np.zeros((m, 3), np.float64)
    np.add.at(cen, inverse, p.astype(np.float64))
    cen = (cen / counts[:, None]).astype(f32)
    ch = np.stack([(c >> 16) & 255, (c >> 8) & 255, c & 255], -1).astype(np.int64)
    sums = np.zeros((m, 3), np.int64)
    np.add.at(sums, inverse, ch)
    mean = (sums.astype(f32) / counts.astype(f32)[:, None]).astype(np.int64)  # truncated
    return cen, ((mean[:, 0] << 16) | (mean[:, 1] << 8) | mean[:, 2]).astype(np.uint32)


def _sequential_sum(a):
    """row sums of a 2-D array, one addition after the other in the array's dtype and in index order: PCL's loop is a plain
    running sum.  (ndarray.sum adds pairwise: in float32 that is several times more accurate over rows of hundreds of
    entries than any running float32 sum, the detector's included.)"""
    return np.add.accumulate(a, axis=1)[:, -1]


def octave_scales(scale, nspo):
    f32 = np.float32
    i = np.arange(nspo + 3, dtype=f32)
    scales = (f32(scale) * np.power(f32(2.0), (i - f32(1.0)) / f32(nspo))).astype(f32)
    sigma2 = (scales * scales).astype(f32)
    return scales, sigma2, (f32(9.0) * sigma2).astype(f32)


def sift_pipeline(points, rgb, dtype, min_scale=0.005, nr_octaves=5, nspo=5, min_contrast=0.001):
    """dict(keypoints: list of (octave, point, column); margins: the smallest decision margin of each; octaves: list of
    dict(cloud, dog, scales, rows (row lengths), k); sizes: every voxel grid's output size; stop: 'gate' or 'count')"""
    f32 = np.float32
    c = rgb.astype(np.uint32)
    words = c[:, 2] | (c[:, 1] << np.uint32(8)) | (c[:, 0] << np.uint32(16))
    cloud = points.astype(f32)
    keypoints, margins, octaves, sizes, stop = [], [], [], [], "count"
    scale = f32(min_scale)
    for o in range(nr_octaves):
        cloud, words = voxel_grid(cloud, words, scale)
        n = len(cloud)
        sizes.append(n)
        if n < MIN_POINTS:
            stop = "gate"
            break
        scales, sigma2, cut = octave_scales(scale, nspo)
        r = np.int64(words >> 16) & 255, np.int64(words >> 8) & 255, np.int64(words) & 255
        inten = (299 * r[0] + 587 * r[1] + 114 * r[2]).astype(dtype) / dtype(1000.0)
        d = cloud[:, None, :] - cloud[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(f32) + d[..., 2] * d[..., 2]
        assert d2.dtype == f32
        radius = f32(3.0) * scales[-1]
        in_row = d2 < f32(np.float64(radius) * np.float64(radius))
        resp = np.zeros((n, len(scales)), dtype)
        for s in range(len(scales)):
            take = in_row & (d2 <= cut[s])
            w = np.where(take, np.exp(dtype(-0.5) * d2.astype(dtype) / dtype(sigma2[s])), dtype(0))
            resp[:, s] = _sequential_sum(w * inten[None, :]) / _sequential_sum(w)
        dog = resp[:, 1:] - resp[:, :-1]
        k = min(NEIGHBOURS, n)
        nbr = np.argsort(d2, axis=1, kind="stable")[:, :k]
        col = dog[nbr]                      # (n, k, columns)
        srt = np.sort(col, axis=1)
        mn, mx = srt[:, 0, :], srt[:, -1, :]
        for i in range(n):
            for s in range(1, dog.shape[1] - 1):
                v = dog[i, s]
                if not abs(v) >= f32(min_contrast):
                    continue
                if v == mn[i, s] and v < mn[i, s - 1] and v < mn[i, s + 1]:
                    gaps = [mn[i, s - 1] - v, mn[i, s + 1] - v, (srt[i, 1, s] - v) if k > 1 else np.inf]
                elif v == mx[i, s] and v > mx[i, s - 1] and v > mx[i, s + 1]:
                    gaps = [v - mx[i, s - 1], v - mx[i, s + 1], (v - srt[i, -2, s]) if k > 1 else np.inf]
                else:
                    continue
                keypoints.append((o, i, s))
                margins.append(float(min(gaps + [abs(v) - float(f32(min_contrast))])))
        octaves.append(dict(cloud=cloud, dog=dog, scales=scales, rows=in_row.sum(1), k=k))
        scale = f32(scale * f32(2.0))
    return dict(keypoints=keypoints, margins=np.array(margins), octaves=octaves, sizes=sizes, stop=stop)
