"""Frames, tile heights, batches and pyramid shapes of tests/test_gpu_pyramid_tiles.py; tests/test_pyramid_plan_cpu.py checks
that every one of them gets a fused plan in both LDS layouts (no silent per-level launches on the GPU)."""

# (width, height, pyr_rows or -1, images, levels, scale factor)
CASES = [
    (96, 64, 64, 1, 3, 1.2),     # one tile in each direction (every level must be 40 px or more: three levels at this size)
    (96, 70, 48, 2, 3, 1.2),     # 58 rows of level 1: a few more than one 48-row tile
    (96, 70, 32, 1, 3, 1.2),     # ... and than one 32-row tile
    (160, 144, -1, 1, 8, 1.2),   # the smallest frame with eight levels: level 2 goes over the source, level 3 over level 1
    (300, 144, -1, 9, 8, 1.2),   # 63 quads of level 1: two tile columns, 63 is odd
    (520, 144, 48, 2, 8, 1.2),   # 109 quads: three tile columns (more where 20 KB forces narrower tiles), 109 = 3 * 36 + 1
    (437, 151, -1, 9, 8, 1.2),   # odd sizes, several tiles both ways, the last quad's 8-byte window clamped at sw - 8
    (437, 151, 8, 1, 8, 1.2),    # many short tile rows: halos larger than what a tile owns
    (144, 144, 4, 9, 8, 1.2),    # 4-row tiles own one or two rows of the deep levels
    (437, 151, -1, 9, 4, 1.5),   # 4 levels at 1.5: one group, wide tap windows
    (300, 140, 16, 2, 4, 1.5),
]
