"""Overwrite a batch's matrix pool with a byte pattern between fills.  TEST INFRASTRUCTURE ONLY -- never imported by the product.

The engine recycles its matrix pool without clearing it, and the layouts leave cells that a fill never writes (stripe and lane
padding, cells outside a band, the unused nibble of a direction code, everything behind a z-drop).  `poison(batch, byte)` makes
those cells hold a chosen pattern, so that a reader which lets one of them reach a result is caught (tests/test_gpu_poison.py).

The range comes from dpx_batch_describe: `pool_addr` / `pool_bytes` are the block behind the batch's matrices, and the memset
covers exactly that block.  dpx_batch_create* writes nothing into the pool that a fill relies on: its only hipMemset calls on it are
the guard band's (csrc/dpx_capi.cpp, "if (b->guardBytes) CREATE_TRY(hipMemset(...0xA5...))" and the self-test byte right behind it)
and the timing probe of DPX_TUNE_PLACEMENT on pools of a GiB or more, whose content no kernel reads.  The direction kernels' edge-row
scratch lies inside the same block, behind the codes, and is written by the fill before it is read.  So nothing is re-initialised
after the memset.  Under DPX_POOL_GUARD the memset would wipe the guard band: the helpers refuse to run."""
import ctypes as C
import os

import numpy as np

_H2D, _D2H = 1, 2
SURVIVOR_LIMIT = 64 << 20
_hip = None


def _runtime():
    global _hip
    if _hip is None:
        hip = C.CDLL("libamdhip64.so")   # the runtime the engine itself is linked against
        hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipDeviceSynchronize.argtypes = []
        _hip = hip
    return _hip


def pool_range(batch):
    """(address, bytes) of the batch's matrix pool, checked"""
    assert not os.environ.get("DPX_POOL_GUARD"), "the memset would wipe the guard band behind the matrices"
    d = batch.describe()
    addr, nbytes = int(str(d["pool_addr"]), 16), int(d["pool_bytes"])
    assert addr and addr % 256 == 0 and nbytes > 0, d
    return addr, nbytes


def poison(batch, byte: int) -> None:
    """every byte of the batch's matrix pool becomes `byte`, and none outside it"""
    assert 0 <= byte <= 255
    hip = _runtime()
    addr, nbytes = pool_range(batch)
    assert hip.hipDeviceSynchronize() == 0
    assert hip.hipMemset(addr, byte, nbytes) == 0
    assert hip.hipDeviceSynchronize() == 0
    k = min(64, nbytes)
    for off in (0, nbytes - k):   # the address is right and the memset landed
        back = (C.c_ubyte * k)()
        assert hip.hipMemcpy(back, addr + off, k, _D2H) == 0
        assert bytes(back) == bytes([byte]) * k, (hex(addr), nbytes, off)


def survivors(batch, byte: int, first_bytes=None) -> int:
    """how many int16 words of the pool still hold the pattern (after a fill: the words no kernel wrote, and the few it wrote alike);
    `first_bytes`: count only in that many bytes at the pool's start (the matrices themselves, without the allocation's headroom)"""
    hip = _runtime()
    addr, nbytes = pool_range(batch)
    assert nbytes <= SURVIVOR_LIMIT, nbytes
    assert hip.hipDeviceSynchronize() == 0
    back = np.empty(nbytes // 2, np.uint16)
    assert hip.hipMemcpy(back.ctypes.data, addr, back.nbytes, _D2H) == 0
    if first_bytes is not None:
        assert 0 <= first_bytes <= nbytes
        back = back[:first_bytes // 2]
    return int(np.count_nonzero(back == np.uint16(byte * 0x0101)))
