"""The column tables of the paired-tails block 1 strip kernel (mmla_audio_amd/csrc/rbs_tp.hip), restated
in Python and checked for what the kernel relies on (no GPU).  Block 1's image is 151 = 9 x 16 + 7 columns
wide; workgroups 0 .. 9 n - 1 are the full strips (clip b // 9, strip b % 9), workgroup 9 n + p holds the
7-column tails of clips 2p (part 0) and 2p + 1 (part 1; absent when n is odd and p the last pair):

  ring column x (18)   part = x >= 9, image column 143 + x - 9 part   (151 = W: the zero padding)
  tile column c (16)   part = c >= 8; tap dx reads ring column c + dx (part 0), c + 1 + dx (part 1);
                       the junk columns 7 and 15 read the zero ring column of their half (8, 17)
  pool window w (8)    part = w >= 4, conv columns 144 + 2 (w - 4 part), + 1 -> pooled column 72 + w - 4 part

Checked: every pooled output of 2 and of 3 clips is produced exactly once; every live tile column reads,
for tap dx, the ring column that holds image column (its own - 1 + dx) of its own clip; no lane of one part
reads a ring column of the other; a junk column reads zero columns only; the workgroup count."""
import pytest

H, W, TW, XW = 128, 151, 16, 18
FS = W // TW                      # full strips per clip
WP = (W + 1) // 2                 # pooled width


def grid(n):
    return FS * n + (n + 1) // 2


def workgroup(b, n):
    """-> (pair, clip, w0, has_b)"""
    if b < FS * n:
        return False, b // FS, (b % FS) * TW, False
    clip = 2 * (b - FS * n)
    return True, clip, FS * TW, clip + 1 < n


def ring_col(pair, w0, has_b, x):
    """-> (part, image column, inside the image and of a clip that exists)"""
    part = int(pair and x >= XW // 2)
    iw = w0 - 1 + x - part * (XW // 2)
    return part, iw, 0 <= iw < W and (not part or has_b)


def tile_ring(pair, c, dx):
    if not pair:
        return c + dx
    p, cl = int(c >= TW // 2), c % (TW // 2)
    return p * (XW // 2) + (XW // 2 - 1 if cl == TW // 2 - 1 else cl + dx)


def window(pair, clip, w0, has_b, w):
    """-> (clip, pooled column, the window's second conv column is cut) or None: nothing stored"""
    op = int(pair and w >= 4)
    cc = w0 + 2 * (w - 4 * op)
    if cc >= W or (op and not has_b):
        return None
    return clip + op, (w0 >> 1) + w - 4 * op, cc + 1 >= W


def test_workgroup_count():
    assert [grid(n) for n in (1, 2, 3, 5)] == [10, 19, 29, 48]
    assert grid(16384) == 155648 and 10 * 16384 == 163840


@pytest.mark.parametrize('n', [2, 3])
def test_every_output_is_produced_exactly_once(n):
    seen = {}
    for b in range(grid(n)):
        pair, clip, w0, has_b = workgroup(b, n)
        assert 0 <= clip < n
        for w in range(8):
            o = window(pair, clip, w0, has_b, w)
            if o is None:
                continue
            oc, col, cut = o
            assert 0 <= oc < n and 0 <= col < WP
            assert cut == (col == WP - 1)          # only the clip's last window is cut ('same' pool, odd width)
            assert (oc, col) not in seen, (b, w, seen[(oc, col)])
            seen[(oc, col)] = (b, w)
    assert len(seen) == n * WP


@pytest.mark.parametrize('n', [2, 3])
def test_taps_read_their_own_clip_s_columns(n):
    for b in range(grid(n)):
        pair, clip, w0, has_b = workgroup(b, n)
        for c in range(TW):
            part = int(pair and c >= TW // 2)
            junk = pair and c % (TW // 2) == TW // 2 - 1
            out_col = w0 + c - part * (TW // 2)            # the conv output column of a live tile column
            for dx in range(3):
                x = tile_ring(pair, c, dx)
                assert 0 <= x < XW
                rp, iw, ok = ring_col(pair, w0, has_b, x)
                assert rp == part, (b, c, dx)              # never the other part's ring half
                if junk:
                    assert not ok and iw == W              # the zero column of its own half
                elif out_col < W:
                    assert iw == out_col - 1 + dx
                    assert ok == (0 <= iw < W and (not part or has_b))
            if pair and not junk:
                assert out_col < W


def test_shortcut_pixel_is_the_window_s_top_left():
    """a window's shortcut pixel (lane n: window n >> 2) is the first conv column of the window it is added to"""
    for n in (2, 3):
        for b in range(grid(n)):
            pair, clip, w0, has_b = workgroup(b, n)
            for w in range(8):
                sc_part = int(pair and w >= 4)
                sc_col = w0 + 2 * (w - 4 * sc_part)
                o = window(pair, clip, w0, has_b, w)
                if o is not None:
                    assert (clip + sc_part, sc_col // 2) == o[:2] and sc_col < W
