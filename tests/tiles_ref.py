"""NumPy restatement of the pixel side (include/paths_hip.h: paths_grey_histogram, paths_tile_tissue, paths_tile_compact,
paths_tiles_to_input, paths_scatter_rows; paths_amd.pixels) as plain array code.  Deliberately independent of paths_amd.pixels.

It is the CONTRACT, not a comparison with a library: the reference reaches its tissue mask through tiatoolbox's OtsuTissueMasker
(OpenCV's 8-bit RGB2GRAY, then Otsu's threshold), and neither cv2, skimage nor tiatoolbox is installed where these tests run.

An image is uint8 [rows, cols, 3] RGB; tiles are uint8 [n, P, P, 3]; cell (x, y) of a level image covers rows x P .. x P + P - 1 and
columns y P .. y P + P - 1."""
import numpy as np


def grey(rgb):
    """OpenCV's 8-bit RGB2GRAY: (4899 R + 9617 G + 1868 B + 8192) >> 14, in integers."""
    p = np.asarray(rgb).astype(np.int64)
    return (4899 * p[..., 0] + 9617 * p[..., 1] + 1868 * p[..., 2] + 8192) >> 14


def histogram(images):
    """int64 [256] over all pixels of all images, jointly."""
    counts = np.zeros(256, np.int64)
    for im in images:
        counts += np.bincount(grey(im).reshape(-1), minlength=256)
    return counts


def between_class(counts, t):
    """w0 w1 (s0 / w0 - s1 / w1)^2 of the classes {g <= t} / {g > t}: exact integer counts and sums converted to float64, every
    operation rounded separately."""
    c = [int(v) for v in counts]
    w0, w1 = sum(c[:t + 1]), sum(c[t + 1:])
    s0, s1 = sum(g * c[g] for g in range(t + 1)), sum(g * c[g] for g in range(t + 1, 256))
    d = np.float64(s0) / np.float64(w0) - np.float64(s1) / np.float64(w1)
    return np.float64(w0) * np.float64(w1) * (d * d)


def otsu(counts):
    """The first t in [gmin, gmax - 1] with the largest between_class; gmin for a constant image."""
    occupied = np.nonzero(np.asarray(counts))[0]
    gmin, gmax = int(occupied[0]), int(occupied[-1])
    if gmin == gmax:
        return gmin
    values = [between_class(counts, t) for t in range(gmin, gmax)]
    return gmin + int(np.argmax(values))                 # (argmax: the first of equal maxima)


def passing_count(size, tissue_threshold):
    """The smallest count with count / size > tissue_threshold in float64 (size + 1: none passes)."""
    ok = np.arange(size + 1) / size > tissue_threshold
    return int(np.argmax(ok)) if ok.any() else size + 1


def lattice(P, stride):
    return np.arange(P // stride) * stride + stride // 2


def tissue_counts(tiles, threshold, stride):
    """int32 [n]: lattice pixels with g < threshold (strict)."""
    tiles = np.asarray(tiles)
    at = lattice(tiles.shape[1], stride)
    g = grey(tiles[:, at][:, :, at])
    return (g < threshold).sum(axis=(1, 2)).astype(np.int32)


def tissue(tiles, threshold, tissue_threshold=0.1, stride=4):
    """counts, flags, order (the first m entries), m, slots - flags by the reference's own float64 comparison."""
    counts = tissue_counts(tiles, threshold, stride)
    size = (np.asarray(tiles).shape[1] // stride) ** 2
    flags = (counts / size > tissue_threshold).astype(np.uint8)
    order = np.nonzero(flags)[0].astype(np.int32)                  # stable: request order
    slots = np.full(len(flags), -1, np.int32)
    slots[order] = np.arange(len(order), dtype=np.int32)
    return counts, flags, order, len(order), slots


def round_to(values, kind):
    """float32 values rounded to nearest even into ``kind`` ("float32", "float16", "bfloat16"), returned as float32."""
    v = np.asarray(values, np.float32)
    if kind == "float32":
        return v
    if kind == "float16":
        return v.astype(np.float16).astype(np.float32)
    bits = v.view(np.uint32).astype(np.uint64)
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000       # (finite values only: the tables hold no NaN)
    return bits.astype(np.uint32).view(np.float32)


def to_tensor_table(kind):
    """[3, 256]: v / 255 in float32, then the cast."""
    v = np.arange(256, dtype=np.float32) / np.float32(255)
    return round_to(np.broadcast_to(v, (3, 256)).copy(), kind)


def normalize_table(mean, std, kind):
    """[3, 256]: (v / 255 - mean[c]) / std[c] in float32, then the cast."""
    v = np.arange(256, dtype=np.float32) / np.float32(255)
    m, s = np.asarray(mean, np.float32).reshape(3, 1), np.asarray(std, np.float32).reshape(3, 1)
    return round_to((v[None, :] - m) / s, kind)


def encoder_input(tiles, order, first, count, table):
    """float32 [count, 3, P, P]: table[c][byte c] of tiles order[first .. first + count)."""
    picked = np.asarray(tiles)[np.asarray(order)[first:first + count]]           # [count, P, P, 3]
    out = np.empty((count, 3) + picked.shape[1:3], np.float32)
    for c in range(3):
        out[:, c] = table[c][picked[..., c]]
    return out


def scatter_rows(encoded, slots, dim, dtype):
    """[n, dim] in dtype: encoded[slots[k]] cast once, or +0."""
    out = np.zeros((len(slots), dim), dtype)
    hit = np.asarray(slots) >= 0
    if hit.any():
        with np.errstate(over="ignore"):                              # (a value beyond the target's range becomes an infinity)
            out[hit] = np.asarray(encoded)[np.asarray(slots)[hit]].astype(dtype)
    return out


def cell_tiles(image, P, cells=None):
    """uint8 [n, P, P, 3]: the windows of ``cells`` ([n, 2]; None: every cell, row-major) of a level image."""
    image = np.asarray(image)
    X, Y = image.shape[0] // P, image.shape[1] // P
    if cells is None:
        cells = np.stack(np.meshgrid(np.arange(X), np.arange(Y), indexing="ij"), axis=-1).reshape(-1, 2)
    return np.stack([image[x * P:(x + 1) * P, y * P:(y + 1) * P] for x, y in np.asarray(cells)])


def encode_level(image, P, threshold, table, model, dim, dtype, tissue_threshold=0.1, stride=4):
    """The grid [X, Y, dim] of ONE level over ALL its cells: model(float32 [m, 3, P, P]) -> [m, dim] for the tissue tiles, +0 rows for
    the others."""
    tiles = cell_tiles(image, P)
    _, _, order, m, slots = tissue(tiles, threshold, tissue_threshold, stride)
    encoded = model(encoder_input(tiles, order, 0, m, table)) if m else None
    rows = scatter_rows(encoded, slots, dim, dtype)
    return rows.reshape(image.shape[0] // P, image.shape[1] // P, dim)
