"""The buffer pool of pipeline.TileEngine and planes that die inside a reference cycle: a DevicePlane and its DeviceBuffer that
are collected together are finalised in either order -- the plane gives the buffer back, the buffer frees itself -- and the
pool must never hand such a buffer out again (it did: the run after a refused product run met a NULL address)."""
import gc

import numpy as np
import pytest

from proteus_amd import _capi, pipeline

pytestmark = pytest.mark.gpu


def test_planes_collected_in_a_cycle_leave_no_freed_buffer_in_the_pool():
    ctx = _capi.Context(0)
    engine = pipeline.TileEngine(ctx)
    try:
        gc.collect()
        gc.disable()                                      # the cycles below die in the one collection this test asks for
        try:
            for _ in range(6):
                plane = engine.upload(np.arange(100, dtype=np.uint8).reshape(10, 10))
                holder = {'plane': plane}
                holder['self'] = holder                   # a cycle, as the frames of a refused run under their traceback
                del plane, holder
            gc.collect()
        finally:
            gc.enable()
        taken = [engine.plane((10, 10), np.uint8) for _ in range(8)]
        assert all(p.ptr for p in taken) and len({p.ptr for p in taken}) == len(taken)
        again = engine.upload(np.full((10, 10), 7, dtype=np.uint8))
        assert again.ptr and (again.numpy() == 7).all()
        dead = engine.plane((4, 4), np.uint8)
        buf = dead.buf
        buf.free()                                        # a buffer that freed itself first: giving it back is a no-op
        dead.release()
        assert all(b.ptr for bufs in engine._free.values() for b in bufs)
    finally:
        engine.close()
        ctx.close()
