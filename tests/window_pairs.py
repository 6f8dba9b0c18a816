"""The work list of the persistent window-attention kernel (csrc/attention_win2.hip: attn_win14p_kernel / launch_win14) restated as
pure functions, and the chooser of test shapes that make its workgroups walk several (window, head) pairs per launch.

The launcher starts min(npairs, CUs) workgroups; workgroup x runs the pairs x, x + gridDim.x, ... one after the other and carries
its K / V ring (three slots, seven key tiles per pair), its two row-offset tables (pair parity) and the prefetched query rows of
the next pair across the pair boundaries.  tests/test_attention_window_pairs_cpu.py checks the chooser;
tests/test_attention_window_pairs_gpu.py runs the shapes it picks."""
from dataclasses import dataclass
from typing import List, Tuple

WINDOW = 14
HEAD_CHOICES = (3, 5, 7)


@dataclass(frozen=True)
class Schedule:
    cus: int
    G: int
    heads: int
    B: int

    @property
    def nwx(self) -> int:
        return -(-self.G // WINDOW)

    @property
    def nwin(self) -> int:
        return self.nwx * self.nwx

    @property
    def npairs(self) -> int:
        return self.heads * self.B * self.nwin

    @property
    def wgs(self) -> int:
        return min(self.npairs, self.cus)

    def pair(self, p: int) -> Tuple[int, int, int]:
        """pair number -> (image, head, window)"""
        seq = p // self.heads
        return seq // self.nwin, p % self.heads, seq % self.nwin

    def items(self, x: int) -> List[int]:
        """the pairs of workgroup x, in the order it runs them"""
        return list(range(x, self.npairs, self.wgs))

    def place(self, p: int) -> Tuple[int, int]:
        """pair number -> (workgroup, position k among that workgroup's items)"""
        return p % self.wgs, p // self.wgs

    def padded(self, window: int) -> bool:
        """whether the window holds pad tokens: the last row / column of windows of a map that is no multiple of 14"""
        if self.G % WINDOW == 0:
            return False
        wy, wx = divmod(window, self.nwx)
        return wy == self.nwx - 1 or wx == self.nwx - 1

    def counts(self) -> List[int]:
        """the distinct numbers of pairs per workgroup, ascending"""
        return sorted({len(self.items(x)) for x in range(self.wgs)})

    def describe(self, p: int) -> str:
        b, h, w = self.pair(p)
        x, k = self.place(p)
        return (f"pair {p}: image {b}, head {h}, window {w} ({'padded' if self.padded(w) else 'full'}), "
                f"workgroup {x}, item k = {k} of {len(self.items(x))}")


def properties(s: Schedule) -> dict:
    """(a) workgroups run exactly n or n + 1 pairs, n >= 3, both counts occur: both row-offset tables are reused, a pair starts in each
           of the three ring slots and the first slot comes round again;
       (b) some workgroup changes head between consecutive pairs;
       (c) some workgroup goes from a padded window to a full one, and some from a full one to a padded one."""
    cnt = s.counts()
    a = len(cnt) == 2 and cnt[1] == cnt[0] + 1 and cnt[0] >= 3
    b = pad_full = full_pad = False
    for x in range(s.wgs):
        it = s.items(x)
        for p, q in zip(it, it[1:]):
            (_, hp, wp), (_, hq, wq) = s.pair(p), s.pair(q)
            b |= hp != hq
            pad_full |= s.padded(wp) and not s.padded(wq)
            full_pad |= not s.padded(wp) and s.padded(wq)
    return {"a": a, "b": b, "c": pad_full and full_pad, "counts": cnt}


def wanted(s: Schedule) -> bool:
    pr = properties(s)
    return pr["a"] and pr["b"] and (pr["c"] or s.G % WINDOW == 0)


def smallest_batch(cus: int, G: int, heads: int) -> int:
    """the smallest batch with npairs >= 3.5 * cus and npairs % cus != 0"""
    per_image = Schedule(cus, G, heads, 1).npairs
    B = 1
    while B * per_image < 3.5 * cus or (B * per_image) % cus == 0:
        B += 1
    return B


def choose(cus: int, G: int) -> Tuple[int, int]:
    """(cus, G) -> (heads, B): per head count the smallest batch of smallest_batch(); the first head count of (3, 5, 7) whose schedule
    has (a), (b) and -- on a map that is no multiple of 14 -- (c)."""
    for heads in HEAD_CHOICES:
        B = smallest_batch(cus, G, heads)
        if wanted(Schedule(cus, G, heads, B)):
            return heads, B
    raise ValueError(f"no head count of {HEAD_CHOICES} mixes heads and windows on {cus} workgroups at G = {G}")
