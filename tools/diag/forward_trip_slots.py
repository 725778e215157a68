"""How many list slots the forward blend walks on the bench scene, with NULL-padded trips of 8 and with a last trip sized to
what is left (CPU only: the oracle's lists, no GPU).

render_forward.hip: a wave owns one 8x4 pixel block of its tile and walks, in every 64-entry chunk of the tile's list, the
entries whose block mask has the wave's bit, two per pair.  With trips of FWD_PAIRS = 4 pairs only, the last trip of every
(chunk, wave) walk is padded to 8 slots with the NULL entry; with a last trip of 4, 2 or 1 pairs by remainder (full trips
while more than 4 bits remain, 2 pairs for 3-4, 1 pair for 1-2) a NULL slot only fills the second entry of the last pair.

The shipped lists are rebuilt from the oracle's (= the fork's 3-sigma rectangle lists) by preprocess.hip's tests (tight
extent rectangle; the tile / ellipse test with its margins on rectangles of up to GIP_MASK_TILES tiles), the block bits
by the kernel's extent test AND its distance bound.  Early termination (a wave leaves its walk once all its pixels are opaque) is
NOT modelled: the counts are the walk of a scene in which no pixel terminates, an upper bound for both variants.

  python tools/diag/forward_trip_slots.py            # 100k human cloud, the four train_cameras(4, seed=42) views, 1024^2
  P=20000 VIEWS=1 python tools/diag/forward_trip_slots.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scenes  # noqa: E402
from oracle.oracle import RasterOracle  # noqa: E402

P, H, W = int(os.environ.get("P", 100000)), 1024, 1024
VIEWS = int(os.environ.get("VIEWS", 4))
PAIRS = 4
MASK_TILES = 32      # gip_internal.h: GIP_MASK_TILES


def slots_padded(bits):
    """slots walked in trips of 2 * PAIRS, the last one padded"""
    return (bits + 2 * PAIRS - 1) // (2 * PAIRS) * (2 * PAIRS)


def trips_and_slots_tail(bits):
    """full trips while more than PAIRS bits remain, then one trip of 2 pairs (3-4 bits left) or 1 pair (1-2 left)"""
    full = np.where(bits > PAIRS, (bits - PAIRS - 1) // (2 * PAIRS) + 1, 0)          # trips taken while bits > PAIRS
    left = np.maximum(bits - full * 2 * PAIRS, 0)
    tail = np.where(left > 2, 4, np.where(left > 0, 2, 0))
    return full + (left > 0), full * 2 * PAIRS + tail


def view_counts(sc, cam):
    ro = RasterOracle()
    ro.forward(image_height=H, image_width=W, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=np.zeros(3, np.float32),
               scale_modifier=1.0, viewmatrix=cam["viewmatrix"], projmatrix=cam["projmatrix"], sh_degree=0, campos=cam["campos"],
               means3D=sc["means3D"], shs=sc["shs"], opacities=sc["opacities"], scales=sc["scales"], rotations=sc["rotations"])
    g = ro.geom()
    keys, vals, ranges, tt, nc = ro.binning()
    tiles_x = W // 16
    tile_of = (keys >> np.uint64(32)).astype(np.int64)
    gi = vals.astype(np.int64)
    cx = g["means2D"][gi, 0].astype(np.float64) - (tile_of % tiles_x) * 16.0
    cy = g["means2D"][gi, 1].astype(np.float64) - (tile_of // tiles_x) * 16.0
    A, B, C, o = (g["conic_opacity"][gi, k].astype(np.float64) for k in range(4))
    t2 = 2.0 * np.log(255.0 * o) + 0.02
    det = A * C - B * B
    ok = (t2 > 0) & (det > 0)
    inv = np.where(ok, t2 / np.where(det > 0, det, 1.0), 0.0)
    # the shipped lists (preprocess.hip): the tiles of the tight extent rectangle inside the fork's; when that rectangle has 2 ..
    # GIP_MASK_TILES tiles, only those whose pixel box, grown by 0.05 px, the ellipse of 1.02 t2 reaches
    ca, cc = C / np.where(det > 0, det, 1.0), A / np.where(det > 0, det, 1.0)           # cov_xx, cov_yy
    ex, ey = np.sqrt(np.maximum(t2 * ca, 0.0)) * 1.01 + 0.05, np.sqrt(np.maximum(t2 * cc, 0.0)) * 1.01 + 0.05
    mx, my = g["means2D"][gi, 0].astype(np.float64), g["means2D"][gi, 1].astype(np.float64)
    tx, ty = tile_of % tiles_x, tile_of // tiles_x
    tx0, tx1 = np.floor((mx - ex) / 16), np.floor((mx + ex) / 16)
    ty0, ty1 = np.floor((my - ey) / 16), np.floor((my + ey) / 16)
    in_rect = ok & (tx >= tx0) & (tx <= tx1) & (ty >= ty0) & (ty <= ty1)
    area = np.zeros(g["means2D"].shape[0], np.int64)
    np.add.at(area, gi[in_rect], 1)                               # the oracle's list has every tile of the fork's rectangle
    X0, X1, Y0, Y1 = -0.05 - cx, 15.05 - cx, -0.05 - cy, 15.05 - cy

    def q(x, y):
        return A * x * x + 2 * B * x * y + C * y * y
    inside = (X0 <= 0) & (X1 >= 0) & (Y0 <= 0) & (Y1 >= 0)
    cand = [q(xe, np.clip(-B * xe / C, Y0, Y1)) for xe in (X0, X1)] + [q(np.clip(-B * ye / A, X0, X1), ye) for ye in (Y0, Y1)]
    reached = np.where(inside, 0.0, np.minimum.reduce(cand)) <= 1.02 * t2
    masked = (area[gi] > 1) & (area[gi] <= MASK_TILES)
    kept = in_rect & (reached | ~masked)
    # block bits of the kept entries: the kernel's extent test and distance bound
    hx = np.sqrt(inv * C) * 1.01 + 0.05
    hy = np.sqrt(inv * A) * 1.01 + 0.05
    hd = 0.5 * (A - C)
    lmax = 0.5 * (A + C) + np.sqrt(hd * hd + B * B)
    rad = np.sqrt(inv * lmax) * 1.01 + 0.05
    bits = np.zeros((gi.shape[0], 8), bool)
    for b in range(8):
        x0, y0 = 8.0 * (b & 1), 4.0 * (b >> 1)
        ex = np.maximum(np.maximum(x0 - cx, cx - (x0 + 7.0)), 0.0)
        ey = np.maximum(np.maximum(y0 - cy, cy - (y0 + 3.0)), 0.0)
        cols = (cx - hx <= 7.0) if (b & 1) == 0 else (cx + hx >= 8.0)
        bits[:, b] = kept & cols & (cy - hy <= y0 + 3.0) & (cy + hy >= y0) & (ex * ex + ey * ey <= rad * rad)
    # position of every kept entry in its tile's kept list -> chunk; bits per (tile, chunk, wave)
    kt, kb = tile_of[kept], bits[kept]
    first = np.searchsorted(kt, kt, side="left")                  # the oracle's lists are sorted by tile
    chunk = (np.arange(kt.shape[0]) - first) // 64
    walk = kt * 1024 + chunk                                      # < 1024 chunks per tile
    uniq, inv_w = np.unique(walk, return_inverse=True)
    per_walk = np.zeros((uniq.shape[0], 8), np.int64)
    np.add.at(per_walk, inv_w, kb.astype(np.int64))
    lens = np.bincount(kt)
    return dict(entries=int(kept.sum()), live_tiles=int((lens > 0).sum()), longest=int(lens.max()), chunks=int(uniq.shape[0]),
                per_walk=per_walk.reshape(-1))


def main():
    sc = scenes.make_scene("human", P, seed=42, sh_degree=0)
    cams = scenes.train_cameras(4, seed=42, H=H, W=W)[:VIEWS]
    tot = dict(entries=0, live_tiles=0, chunks=0)
    longest, walks = 0, []
    for cam in cams:
        c = view_counts(sc, cam)
        for k in tot:
            tot[k] += c[k]
        longest = max(longest, c["longest"])
        walks.append(c["per_walk"])
    bits = np.concatenate(walks)
    nonempty = bits > 0
    trips_now = (bits + 2 * PAIRS - 1) // (2 * PAIRS)
    trips_tail, slots_tail = trips_and_slots_tail(bits)
    n_bits = int(bits.sum())
    print("%d Gaussians, %d views of %d x %d" % (P, len(cams), W, H))
    print("entries in live tiles                  %10d   (%d live tiles, longest list %d)" % (tot["entries"], tot["live_tiles"], longest))
    print("chunks                                 %10d" % tot["chunks"])
    print("(chunk, wave) walks                    %10d   (%.0f %% non-empty)" % (bits.shape[0], 100.0 * nonempty.mean()))
    print("set bits                               %10d   (%.2f blocks per entry, %.2f bits per non-empty walk)"
          % (n_bits, n_bits / tot["entries"], n_bits / max(int(nonempty.sum()), 1)))
    print("trips, padded / sized last trip        %10d / %d" % (int(trips_now.sum()), int(trips_tail.sum())))
    print("slots walked, padded trips of %d        %10d   (%.3f x bits)" % (2 * PAIRS, int(slots_padded(bits).sum()), slots_padded(bits).sum() / n_bits))
    print("slots walked, last trip of 4 / 2 / 1   %10d   (%.3f x bits, %.1f %% fewer)"
          % (int(slots_tail.sum()), slots_tail.sum() / n_bits, 100.0 * (1.0 - slots_tail.sum() / slots_padded(bits).sum())))
    left = np.where(bits > PAIRS, bits - ((bits - PAIRS - 1) // (2 * PAIRS) + 1) * 2 * PAIRS, bits)      # <= 0: padded full trip
    kinds = [("ends with a full trip", nonempty & (left <= 0)), ("2-pair last trip", left > 2), ("1-pair last trip", (left > 0) & (left <= 2))]
    for name, sel in kinds:
        print("  walks whose chunk %-22s %10d" % (name, int(sel.sum())))


if __name__ == "__main__":
    main()
