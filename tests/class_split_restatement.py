"""A numpy restatement of the class split (include/pvnet_classes.h, pvnet_amd/csrc/class_split.hip): from a label image to what the
voting library's mask kernel would have written for every mask ``labels[i] == k + 1`` -- the bit words, the counts per 4096-pixel
segment, and the cumulative histograms of the thinning bins of every (class, segment) that has pixels.  Written from the header's
text; the RNG and the bin table are the oracle's (oracle/ransac_voting_oracle.py), which restates pvnet_rng.h."""
import numpy as np

from oracle import ransac_voting_oracle as O

SEG_PIXELS = 4096
THIN_BINS = (O.THIN_LAST + 1 + 127) // 128 * 128   # 1536


def class_of(labels: np.ndarray, num_classes: int) -> np.ndarray:
    """1 .. num_classes - 1, or 0 for nobody's: the label's full value decides (a float label has to EQUAL the class)"""
    lab = np.asarray(labels)
    if lab.dtype == np.bool_:
        lab = lab.astype(np.int64)
    if lab.dtype.kind == "f":
        ok = np.isfinite(lab) & (lab >= 1) & (lab < num_classes) & (lab == np.floor(lab))
    else:
        ok = (lab >= 1) & (lab < num_classes)
    return np.where(ok, np.where(ok, lab, 0).astype(np.int64), 0)


def argmax_first(seg: np.ndarray) -> np.ndarray:
    """torch.argmax over axis 1: the first maximum wins, a NaN counts as the maximum (the first NaN wins)"""
    seg = np.asarray(seg, np.float32)
    best, arg = seg[:, 0].copy(), np.zeros(seg[:, 0].shape, np.int64)
    for c in range(1, seg.shape[1]):
        x = seg[:, c]
        with np.errstate(invalid="ignore"):
            take = ~np.isnan(best) & ~(x <= best)
        best, arg = np.where(take, x, best), np.where(take, c, arg)
    return arg


def thin_bins(r: np.ndarray) -> np.ndarray:
    """O.thin_bin for an array of 32-bit words"""
    r = r.astype(np.uint64)
    out = np.zeros(r.shape, np.int64)
    lin = (r >> np.uint64(26)) != 0
    out[lin] = O.THIN_LOG_BINS - 16 + (r[lin] >> np.uint64(22)).astype(np.int64)
    rest = ~lin & (r != 0)
    rr = r[rest]
    e = np.floor(np.log2(rr.astype(np.float64))).astype(np.int64)   # exact below 2^26
    sub = np.where(e >= 4, (rr >> np.maximum(e - 4, 0).astype(np.uint64)) & np.uint64(15),
                   (rr << np.maximum(4 - e, 0).astype(np.uint64)) & np.uint64(15)).astype(np.int64)
    out[rest] = e * 16 + sub
    return out


def split(labels: np.ndarray, num_classes: int, max_num: int, seed: int, image_base: int = 0):
    """labels [b,h,w] -> (bits uint64 [B,words], seg0 int32 [B,nseg], cum uint16 [B,nseg,THIN_BINS] or None, has bool [B,nseg]) with
    B = b (num_classes - 1), virtual image v = i (num_classes - 1) + k; ``cum`` rows are defined where ``has`` (elsewhere zero here,
    unwritten on the device); None when max_num >= h w"""
    cls = class_of(labels, num_classes)
    b, h, w = cls.shape
    npix, nk = h * w, num_classes - 1
    words = (npix + 63) // 64
    nseg = (words + 63) // 64
    B = b * nk
    bits = np.zeros((B, words), np.uint64)
    seg0 = np.zeros((B, nseg), np.int32)
    cum = np.zeros((B, nseg, THIN_BINS), np.uint16) if max_num < npix else None
    flat = cls.reshape(b, npix)
    for i in range(b):
        for k in range(nk):
            v = i * nk + k
            m = np.zeros(words * 64, bool)
            m[:npix] = flat[i] == k + 1
            bits[v] = (m.reshape(words, 64).astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(1, dtype=np.uint64)
            pad = np.zeros(nseg * SEG_PIXELS, bool)
            pad[:words * 64] = m
            seg0[v] = pad.reshape(nseg, SEG_PIXELS).sum(1)
            if cum is None:
                continue
            p = np.flatnonzero(m)
            bins = thin_bins(O.rng_u32(seed, O.TAG_SUB, np.uint64((image_base + v) & 0xFFFFFFFF), p.astype(np.uint64)))
            for s in range(nseg):
                sel = bins[(p // SEG_PIXELS) == s]
                if sel.size:
                    cum[v, s] = np.cumsum(np.bincount(sel, minlength=THIN_BINS)).astype(np.uint16)
    return bits, seg0, cum, seg0 > 0


def kept_before(cum_row: np.ndarray, max_num: int, tn0: int) -> int:
    """pixels of a segment that thinning keeps (what the compaction kernel reads of a row): column K - 1, K bins kept"""
    t = ((int(max_num) << 32) + int(tn0) - 1) // int(tn0)
    k = 0 if t == 0 else O.thin_bin(t - 1) + 1
    return int(cum_row[k - 1]) if k > 0 else 0
