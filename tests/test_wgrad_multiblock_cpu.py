"""The fill rule of the multi-block weight-gradient launch (npcd_wgrad_group_blocks, csrc/gemm.hip) through its pure-Python mirror
npcd.hip.elementwise.wgrad_group_blocks_rule, which takes the compute-unit count as an argument, and the parsing of the
NPCD_WGRAD_MULTIBLOCK switch.  No GPU."""
import pytest

from npcd.hip import elementwise as ew


def _tiles(W):
    """256 x 256 output tiles of the four weight gradients of a block of width W: c_qkv, attn.c_proj, c_fc, mlp.c_proj"""
    return sum((N // 256) * (K // 256) for N, K in ((3 * W, W), (W, W), (4 * W, W), (W, 4 * W)))


def test_tiles_per_block():
    assert [_tiles(W) for W in (256, 512, 1024, 2048)] == [12, 48, 192, 768]


@pytest.mark.parametrize("tiles,cus,expect", [
    (192, 256, 4),       # width 1,024: 4 x 192 = 768 tiles = three full rounds
    (768, 256, 1),       # width 2,048: one block is three full rounds
    (48, 256, 0),        # width 512: 4 x 48 = 192 tiles fill 0.75 of a round
    (12, 256, 0),        # width 256
    (192, 192, 1),       # one block is one full round
    (192, 304, 0),       # 304 CUs: 192 / 304 = 0.63, 384 / 608 = 0.63, 576 / 608 = 0.947, 768 / 912 = 0.84 -- none reaches 0.95
])
def test_fill_rule(tiles, cus, expect):
    assert ew.wgrad_group_blocks_rule(tiles, 16, 4, cus) == expect


def test_fill_rule_respects_the_product_limit_and_rejects_nonsense():
    assert ew.wgrad_group_blocks_rule(192, 8, 4, 256) == 0           # two blocks at the most: 384 / 512
    assert ew.wgrad_group_blocks_rule(192, 16, 4, 0) == 0
    assert ew.wgrad_group_blocks_rule(0, 16, 4, 256) == 0
    assert ew.wgrad_group_blocks_rule(192, 16, 0, 256) == 0
    for tiles in range(1, 800, 7):                                   # whatever it returns obeys the rule it states
        G = ew.wgrad_group_blocks_rule(tiles, 16, 4, 256)
        assert 0 <= G <= 4
        if G:
            rounds = -(-G * tiles // 256)
            assert G * tiles >= 0.95 * rounds * 256
            assert all(g * tiles < 0.95 * (-(-g * tiles // 256)) * 256 for g in range(1, G))


def test_switch_parsing():
    from npcd.models.diffusion import fused
    assert fused._parse_wgrad_multiblock(None) == "on" and fused._parse_wgrad_multiblock("") == "on" and fused._parse_wgrad_multiblock("1") == "on"
    assert fused._parse_wgrad_multiblock("0") == "off"
    assert fused._parse_wgrad_multiblock("force") == "force"
    with pytest.raises(ValueError, match="NPCD_WGRAD_MULTIBLOCK"):
        fused._parse_wgrad_multiblock("yes")
