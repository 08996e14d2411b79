"""LDS bank check of conv_f32x_wgrad's general-geometry (GEN = 1) halo reads, per step shape and halo pitch.

tools/tr_banks.py's model: a ds_read_b64_tr_b16 is serviced in two 32-lane halves; a half reads 8 halo rows (one
pixel each), 32 B per row, and is conflict-free iff the rows' (parity, trswz) pairs -- row bits (0, 1, 3) -- are
distinct. Pixel xw_pixel(ks, b, h, q) of a step of rs rows x seg columns sits at halo row (l / seg) pitch + l % seg,
shifted by r pitch + s per tap; padded slots (l >= rs seg) read too. Prints, for every step shape the step rule
gives at the seven widths and every pitch from seg + 2 that keeps the padded slots' reads inside the 144 rows, the
worst rows-per-slot over all taps, k-steps, halves and reads (1 = conflict-free), and the share of reads at each cost.
usage: python tools/xw_gen_banks.py
"""
from collections import Counter

HROWS = 144


def step_rule(H, W):
    """conv_f32x_wgrad.hip's xw_geometry_gen: the divisor seg <= 64 of W with the most pixels, ties to the larger seg"""
    best = None
    for seg in range(1, min(W, 64) + 1):
        if W % seg:
            continue
        rs = max(1, 64 // seg)
        while rs > 1 and H % rs:
            rs -= 1
        if (rs + 2) * (seg + 2) <= HROWS and (best is None or (rs * seg, seg) > (best[1] * best[0], best[0])):
            best = (seg, rs)
    return best


def costs(seg, pitch):
    c = Counter()
    for ks in range(2):
        for half in range(2):
            for h in range(2):
                pix = [ks * 32 + 8 * b + q + 4 * h for b in (2 * half, 2 * half + 1) for q in range(4)]
                base = [(l // seg) * pitch + l % seg for l in pix]
                for tap in range(9):
                    slots = Counter()
                    for r in base:
                        r += (tap // 3) * pitch + tap % 3
                        slots[(r & 1, (r >> 1) & 1, (r >> 3) & 1)] += 1
                    c[max(slots.values())] += 1
    return c


if __name__ == "__main__":
    for W in (224, 112, 56, 28, 14, 7, 64):
        seg, rs = step_rule(W, W)
        for pitch in range(seg + 2, HROWS):
            if (rs + 2) * pitch > HROWS or (63 // seg + 2) * pitch + 63 % seg + 2 >= HROWS:
                break
            c = costs(seg, pitch)
            n = sum(c.values())
            print(f"W {W:3d}  seg {seg:2d} x rs {rs}  pitch {pitch:2d}  worst {max(c)}  "
                  + "  ".join(f"cost {k}: {100 * v // n}%" for k, v in sorted(c.items())))
