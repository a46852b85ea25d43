"""The absorbed cross-attention at d = 384 (tiny / tiny.en, 6 heads), host side: the public predicate wh_xabs_supports and an emulation
of the index math of the 4-wave form of xabs_attn_kernel (csrc/xabs.hip: NW = 4 waves x KSW = 3 k-steps of 32 channels, 768-byte tile
rows, half tiles of 8 x 768 = 6 KB fetched as 2 waves x 3 LDS-DMA pieces of 1 KB), of the 2-wave workgroups of xabs_qk and of the
3 x 4 x 2 k-tile split of xabs_vup.  The constants below restate the kernel's; tests/test_kernel_index_math.py holds the same checks
for the widths that are multiples of 256, by the same criteria.  No GPU."""
from whisperkit_amd import _lib, api

D, H = 384, 6
NW, KSW = 4, 3                      # waves per workgroup, k-steps (= P V row tiles = DMA pieces of 1 KB) per wave
ROWB = D * 2                        # bytes of a tile row
HALF = 8 * ROWB                     # bytes of a half tile (8 keys)
HW = NW // 2                        # waves that fetch one half tile
N_HALVES = 7                        # ring slots
QK_WPB, QK_GRID_X = 2, 3            # xabs_qk: waves per workgroup, workgroups per (head, batch tile)
VUP_KS, VUP_TW = 3, 2               # xabs_vup: K slices (workgroups per head and batch tile), k tiles per wave


def _xswz(key):
    return ((key & 3) << 2) | ((0x78 >> (2 * ((key >> 2) & 3))) & 3)


def test_wh_xabs_supports_truth_table():
    f = _lib.load().wh_xabs_supports
    for d, h in ((384, 6), (512, 8), (768, 12), (1024, 16), (1280, 20)):
        assert f(d, h) == 1 and api.xabsSupports(d, h) is True and api.Session.xabsSupports(d, h) is True, (d, h)
    for d, h in ((128, 2), (256, 4), (640, 10), (896, 14), (1536, 24), (2304, 36), (384, 8), (1280, 16), (0, 0), (-384, -6)):
        assert f(d, h) == 0 and api.xabsSupports(d, h) is False, (d, h)


def test_shape_constants_come_out_even():
    assert NW * KSW * 32 == D and HALF == HW * KSW * 1024 and ROWB % 256 == 0 and HALF % 256 == 0
    assert 4 * NW >= 16 >= H                                  # 4 softmax-owner heads per wave: one head tile
    lds = N_HALVES * HALF + NW * 32 * 17 * 4 + 1024 + 128
    assert lds == 52864 and 3 * lds <= 160 * 1024             # three workgroups per CU


def test_dma_pieces_cover_every_chunk_of_a_tile_once_and_land_where_the_readers_look():
    """issue(): wave w fetches half w >> 1 of a tile; piece p of wave quarter wq = w & 1, lane l writes LDS bytes
    [(wq KSW + p) 1024 + 16 l, + 16) of the half (linear), reading the tile's global byte
    (8 half + row) ROWB + ((slot ^ xswz(8 half + row)) << 4) with row, slot = the LDS position.  A reader of chunk c of tile row `key` looks
    at LDS slot c ^ xswz(key) of row key & 7 of half key >> 3."""
    lds = {}                                     # (half, LDS byte offset of a 16-byte slot) -> global byte offset inside the 16 x ROWB tile
    for wave in range(NW):
        half_w, wq = wave >> 1, wave & (HW - 1)
        for p in range(KSW):
            for lane in range(64):
                o = (wq * KSW + p) * 1024 + lane * 16
                row, slot = o // ROWB, (o % ROWB) >> 4
                assert row < 8 and o + 16 <= HALF
                src = (half_w * 8 + row) * ROWB + ((slot ^ _xswz(half_w * 8 + row)) << 4)
                assert (half_w, o) not in lds
                lds[(half_w, o)] = src
    assert len(lds) == 16 * ROWB // 16
    assert sorted(lds.values()) == list(range(0, 16 * ROWB, 16))          # every 16-byte chunk of the 16 x 768-byte tile exactly once
    for key in range(16):
        for c in range(ROWB // 16):
            assert lds[(key >> 3, (key & 7) * ROWB + ((c ^ _xswz(key)) << 4))] == key * ROWB + c * 16, (key, c)


def test_swizzle_is_conflict_free_at_a_768_byte_row():
    """The criteria of tests/test_kernel_index_math.py: (1) S phase, ds_read_b128, 4 groups of 16 lanes (lane = key | k group << 4), each
    group touches 16 distinct 16-byte bank groups; (2) P V phase, ds_read_b64_tr_b16, each 32-lane half touches 32 distinct 8-byte bank
    pairs.  For every wave, k-step and row tile of the 4 x 3 partition; the half slot (key >> 3) is a multiple of 256 bytes away."""
    for wave in range(NW):
        for j in range(KSW):
            for kg in range(4):
                c = (wave * KSW + j) * 4 + kg
                chunks = {(((key >> 3) * HALF + (key & 7) * ROWB + ((c ^ _xswz(key)) << 4)) >> 4) & 15 for key in range(16)}
                assert len(chunks) == 16, (wave, j, kg)
            for second in (0, 4):
                for half in (0, 1):
                    pairs = set()
                    for lane in range(half * 32, half * 32 + 32):
                        g16, sl = lane >> 4, lane & 15
                        key = (g16 >> 1) * 8 + (sl >> 2) + second
                        c = (wave * KSW + j) * 4 + (g16 & 1) * 2 + ((sl & 3) >> 1)
                        addr = (key >> 3) * HALF + (key & 7) * ROWB + ((c ^ _xswz(key)) << 4) + (sl & 1) * 8
                        pairs.add((addr >> 3) & 31)
                    assert len(pairs) == 32, (wave, j, second, half)


def test_k_steps_and_row_tiles_cover_the_384_channels_once():
    s_cover, pv_cover, part_cover = [], [], []
    for wave in range(NW):
        for j in range(KSW):
            for kg in range(4):                              # S phase: chunk (wave KSW + j) 4 + kg = 8 channels; the Q' fragment of the same lane
                c = (wave * KSW + j) * 4 + kg
                assert c * 8 == wave * KSW * 32 + j * 32 + kg * 8          # xabs_load_qfrag: c0 + 32 j + 8 (lane >> 4)
                s_cover += range(c * 8, c * 8 + 8)
            pv_cover += range((wave * KSW + j) * 32, (wave * KSW + j) * 32 + 32)          # P V: row tile wave KSW + mt
            part_cover += [(wave * KSW + j) * 4 + g for g in range(4)]                     # partial store: c / 8
    assert sorted(s_cover) == sorted(pv_cover) == list(range(D))
    assert sorted(part_cover) == list(range(D // 8))
    # softmax owners: wave = head >> 2, lane = key | (head & 3) << 4 - 16 heads x 16 keys exactly once, the 6 real heads among them
    owners = sorted((4 * wave + (lane >> 4), lane & 15) for wave in range(NW) for lane in range(64))
    assert owners == [(h, k) for h in range(16) for k in range(16)]


def test_qk_and_vup_partitions_cover_their_tiles_once():
    rts = [(bx * QK_WPB + wave) * 2 + s for bx in range(QK_GRID_X) for wave in range(QK_WPB) for s in range(2)]
    assert sorted(rts) == list(range(D // 32))               # xabs_qk: the 12 row tiles of 32 channels
    kts = [(ksi * 4 + wave) * VUP_TW + i for ksi in range(VUP_KS) for wave in range(4) for i in range(VUP_TW)]
    assert sorted(kts) == list(range(D // 16)) and VUP_KS <= 4         # xabs_vup: the 24 k tiles; its ticket combine sums at most 4 slices


def test_key_tail_mask_of_the_last_tile():
    n_tiles = (1500 + 15) // 16
    assert n_tiles == 94 and 1500 - 93 * 16 == 12
    for S in (1, 2, 3, 4):
        edges = [sp * n_tiles // S for sp in range(S + 1)]
        assert edges[0] == 0 and edges[-1] == n_tiles and all(b > a for a, b in zip(edges, edges[1:]))
