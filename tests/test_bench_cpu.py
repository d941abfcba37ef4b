"""bench.py's host side, on CPU: the headline instance drawn by row blocks on several threads is the sequential instance."""
import numpy as np

import bench
from tools import instances


def test_headline_instance_drawn_by_threads_is_the_sequential_instance():
    # bench.uniform_to_device draws the timed input in row blocks on up to 16 threads; every entry must be what
    # tools.instances.uniform_cost_blocks (the instance of the committed goldens) draws in one stream
    n = 1000
    ref = instances.uniform_cost(n)
    for rows, threads in ((64, 4), (1000, 1), (333, 3), (1, 8)):
        got = np.full((n, n), np.nan, np.float32)
        seen = []

        def sink(lo, blk):
            assert blk.dtype == np.float32 and blk.flags.c_contiguous and blk.shape == (min(rows, n - lo), n)
            got[lo:lo + len(blk)] = blk
            seen.append(lo)

        bench.draw_uniform(n, sink, rows=rows, threads=threads)
        assert sorted(seen) == list(range(0, n, rows))
        assert np.array_equal(got, ref), (rows, threads)


def test_a_row_block_on_its_own_is_the_same_rows_of_the_instance():
    n = 777
    ref = instances.uniform_cost(n)
    for lo, h in ((0, 1), (1, 5), (300, 477), (776, 1)):
        blk = bench.uniform_rows(n, lo, np.empty((h, n)), np.empty((h, n), np.float32))
        assert np.array_equal(blk, ref[lo:lo + h])
