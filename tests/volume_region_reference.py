"""Which bricks can a data-volume region update reach? (include/tbrm_volume_region.h)

reached_bricks restates k_brick_minmax's loop (tbrm_volume_kernels.hip) in numpy, texel by texel: brick b is reached when one of
the texels its 9 x 9 x 9 loop addresses lies in the box. rule_bricks is the closed form the library launches its restricted pass
by. tests/test_volume_region_abi.py holds the two against each other; tests/test_gpu_volume_region.py counts with the first."""
import numpy as np

WRAP, CLAMP = 0, 1


def _address(i, n, mode):
    return i % n if mode == WRAP else min(max(i, 0), n - 1)


def reached_bricks(dims, mode, origin, extent):
    """the set of (bx, by, bz) whose min/max k_brick_minmax computes from at least one texel of [origin, origin + extent)"""
    n = dims
    bn = [(d + 7) // 8 for d in n]
    inside = np.zeros((n[2], n[1], n[0]), dtype=bool)
    inside[origin[2]:origin[2] + extent[2], origin[1]:origin[1] + extent[1], origin[0]:origin[0] + extent[0]] = True
    out = set()
    for bz in range(bn[2]):
        for by in range(bn[1]):
            for bx in range(bn[0]):
                hit = False
                for t in range(9 * 9 * 9):
                    dx, dy, dz = t % 9, (t // 9) % 9, t // 81
                    x, y, z = bx * 8 + dx, by * 8 + dy, bz * 8 + dz
                    if x > n[0] or y > n[1] or z > n[2]:   # the +8 tap only exists as the "+1" neighbour of an in-range base tap
                        continue
                    if inside[_address(z, n[2], mode), _address(y, n[1], mode), _address(x, n[0], mode)]:
                        hit = True
                        break
                if hit:
                    out.add((bx, by, bz))
    return out


def rule_bricks(dims, mode, origin, extent):
    """per axis: bricks max(0, ceil((o - 8) / 8)) .. floor((o + e - 1) / 8), and under wrap addressing the axis' last brick when the
    box holds texel 0; the reach is the product of the three axes' sets"""
    axes = []
    for c in range(3):
        o, e, nb = origin[c], extent[c], (dims[c] + 7) // 8
        s = set(range(max(0, -((8 - o) // 8)), min(nb - 1, (o + e - 1) // 8) + 1))
        if mode == WRAP and o == 0:
            s.add(nb - 1)
        axes.append(s)
    return {(bx, by, bz) for bx in axes[0] for by in axes[1] for bz in axes[2]}
