"""The cases shared by test_figure_cpu.py and test_gpu_figure_device.py: seeded random frames and index planes over all
256 byte values, random colour tables, and per case (H, W, d, layout, P, B) chosen for the composer's paths: partial
windows in both directions and canvas padding; d = 1; the largest window sum (d = 16); a d that is no power of two with
a row pitch that is no multiple of 16 and a batch stride; an image smaller than one window; an empty cell; no frames at
all; two panels on one plane; and the remaining vector widths (d = 2, d = 8) with a cut last row of windows."""
import numpy as np

GAP = 16


class Case(object):
    def __init__(self, name, H, W, d, layout, P, B, seed, frames=True, modes=None, alias=None, gap=GAP):
        rng = np.random.default_rng(seed)
        self.name, self.H, self.W, self.d, self.layout, self.P, self.B, self.gap = name, H, W, d, layout, P, B, gap
        self.frames = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8) if frames else None
        self.planes = [rng.integers(0, 256, (B, H, W), dtype=np.uint8) for _ in range(P)]
        # all 256 byte values in every plane where it is large enough, the extremes always
        for pl in self.planes:
            flat = pl.reshape(-1)
            flat[:2] = (0, 255)
            if flat.size >= 512:
                flat[rng.permutation(flat.size)[:256]] = np.arange(256, dtype=np.uint8)
        if alias is not None:                            # panel alias[0] shows the plane of panel alias[1]
            self.planes[alias[0]] = self.planes[alias[1]]
        self.luts = [rng.integers(0, 256, (256, 3), dtype=np.uint8) for _ in range(P)]
        for t in self.luts:
            t[0], t[255] = (255, 255, 255), (0, 0, 0)
        self.modes = list(modes) if modes is not None else [(p + 1) % 2 if frames else 0 for p in range(P)]

    def args(self):
        return self.frames, self.planes, self.luts, self.modes, self.layout, self.d, self.gap


def cases():
    return [
        Case('partial_windows', 37, 53, 4, (2, 2), 4, 1, 1),
        Case('d1', 16, 16, 1, (1, 3), 3, 2, 2),
        Case('d16_largest_sum', 48, 80, 16, (2, 2), 4, 1, 3, modes=[1, 1, 0, 0]),
        Case('d3_pitch_batch', 33, 100, 3, (1, 3), 3, 3, 4),
        Case('smaller_than_a_window', 5, 7, 8, (1, 1), 1, 1, 5),
        Case('empty_cell', 64, 128, 4, (2, 2), 3, 1, 6),
        Case('no_frames', 40, 64, 4, (2, 2), 4, 2, 7, frames=False),
        Case('aliased_planes', 32, 48, 4, (1, 3), 3, 2, 8, alias=(2, 0)),
        Case('d2', 30, 32, 2, (2, 2), 4, 2, 9),
        Case('d8_cut_rows', 20, 48, 8, (1, 3), 3, 1, 10, gap=0),
        Case('gap64_2x1', 18, 32, 4, (2, 1), 2, 1, 11, gap=64),
    ]


def saturated():
    """the largest sum a window can hold: 16 x 16 pixels of 255 through a table of 255, both modes"""
    c = Case('saturated', 16, 32, 16, (1, 2), 2, 1, 12, modes=[1, 0])
    c.frames[:] = 255
    for pl in c.planes:
        pl[:] = 7
    for t in c.luts:
        t[7] = (255, 255, 255)
    return c


def windows(H, W, d):
    """[(y, x, rows slice, columns slice)] of every panel pixel"""
    return [(y, x, slice(y * d, min((y + 1) * d, H)), slice(x * d, min((x + 1) * d, W)))
            for y in range(-(-H // d)) for x in range(-(-W // d))]


def panel_origin(c, p):
    Hp, Wp = -(-c.H // c.d), -(-c.W // c.d)
    return c.gap + (p // c.layout[1]) * (Hp + c.gap), c.gap + (p % c.layout[1]) * (Wp + c.gap), Hp, Wp
