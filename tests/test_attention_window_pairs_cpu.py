"""The shapes tests/test_attention_window_pairs_gpu.py runs, checked without a GPU: the restated work list of the persistent window
kernel (tests/window_pairs.py) and the shape chooser's promise that every workgroup walks three or more pairs that mix heads,
padded and full windows."""
import pytest

import window_pairs as WP


def test_schedule_covers_every_pair_once():
    s = WP.Schedule(cus=256, G=29, heads=3, B=34)
    assert (s.nwx, s.nwin, s.npairs, s.wgs) == (3, 9, 918, 256)
    seen = sorted(p for x in range(s.wgs) for p in s.items(x))
    assert seen == list(range(s.npairs))
    assert s.pair(0) == (0, 0, 0) and s.pair(4) == (0, 1, 1) and s.pair(27) == (1, 0, 0) and s.pair(917) == (33, 2, 8)
    assert s.place(256 + 5) == (5, 1) and s.items(5)[1] == 261
    assert [s.padded(w) for w in range(9)] == [False, False, True, False, False, True, True, True, True]
    assert not any(WP.Schedule(256, 28, 3, 1).padded(w) for w in range(4))
    few = WP.Schedule(cus=256, G=20, heads=2, B=2)                  # fewer pairs than CUs: one pair per workgroup
    assert few.wgs == few.npairs == 16 and few.counts() == [1]


@pytest.mark.parametrize("cus", [256, 304])
@pytest.mark.parametrize("G", [14, 15, 20, 27, 29])
def test_chooser_mixes_pairs(cus, G):
    heads, B = WP.choose(cus, G)
    s = WP.Schedule(cus, G, heads, B)
    pr = WP.properties(s)
    assert s.npairs >= 3.5 * cus and s.npairs % cus != 0
    assert pr["a"] and pr["counts"][0] >= 3, pr
    assert pr["b"], pr
    if G % 14:
        assert pr["c"], pr
    assert heads == 3
    if cus == 256:
        assert B == {14: 299, 15: 75, 20: 75, 27: 75, 29: 34}[G] and 897 <= s.npairs <= 918


def test_chooser_searches_the_head_counts():
    assert WP.choose(120, 20)[0] == 7                               # 120 workgroups: 3 and 5 divide it, a workgroup keeps its head
    assert WP.choose(120, 14) == (7, 60)
    assert not WP.properties(WP.Schedule(120, 20, 3, 36))["b"]
    with pytest.raises(ValueError):
        WP.choose(105, 20)                                          # 3, 5 and 7 all divide 105: no choice changes head, and the chooser says so


def test_encoder_refuses_a_width_between_k_steps():
    """3 heads of 80 = 240: the activation rows would be read at the weights' padded K = 256 (lda = K) -- wrong numbers and reads past the
    buffers' ends.  The engine says so before it touches a weight or the device."""
    from camouflaged_vlm_amd import spec
    from camouflaged_vlm_amd.engine import Precision, SamEncoder
    g = spec.SamGeometry(inp_size=320, embed_dim=240, depth=2, num_heads=3, global_attn_indexes=(1,))
    with pytest.raises(ValueError, match="embed_dim = 240"):
        SamEncoder({}, g, "cpu", Precision.named("exact"))
