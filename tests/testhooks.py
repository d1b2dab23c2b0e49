"""Test infrastructure: the library with the prototypes of the private test-hook headers (quilt_amd/csrc/*_testhook.h) declared
beside the public ones -- quilt_amd.native.declare, the parser lib() applies to include/*.h -- and the callers of
csrc/fullpass_testhook.h that several tests share.  Nothing in the product imports this."""
import ctypes as C
import functools
import os

import numpy as np

from quilt_amd import native


@functools.lru_cache(maxsize=None)
def hook_lib():
    for header in ("fullpass_testhook.h", "impute_testhook.h"):
        native.declare(os.path.join(native.CSRC, header))
    return native.lib()


def last_plan():
    """qa_fullpass_last_plan: the calling thread's last launch set as planned and as carved"""
    out = (C.c_int64 * 6)()
    native.check(hook_lib().qa_fullpass_last_plan(out))
    return dict(zip(("P", "planned", "fixed", "carved", "n_buf", "kind"), (int(v) for v in out)))


def launch_set(dev, gl, flags, cols, K_top, always_normalize):
    """qa_fullpass_launch_set: c, dosage, list pointers / indices / values of one launch set"""
    ptr = native.ptr
    panel = dev.panel
    n, T, G = gl.shape[0], panel.nSNPs, panel.nGrids
    n_thin = int((cols >= 0).sum()) if K_top > 0 else 0
    cap = max(n * n_thin * panel.K, 1)
    bptr = np.zeros(n * max(n_thin, 1) + 1, dtype=np.int32)
    bidx, bval = np.zeros(cap, dtype=np.int32), np.zeros(cap)
    dosage, c = np.zeros((n, T)), np.zeros((n, G))
    native.check(hook_lib().qa_fullpass_launch_set(dev.handle, n, ptr(gl), ptr(np.ascontiguousarray(flags, dtype=np.int32)), ptr(cols),
                                                   K_top, int(always_normalize), ptr(dosage), ptr(c), ptr(bptr), ptr(bidx), ptr(bval), cap))
    total = int(bptr[n * n_thin]) if n_thin else 0
    return dict(c=c, dosage=dosage, list_ptr=bptr[:n * n_thin + 1].copy(), list_idx=bidx[:total].copy(), list_val=bval[:total].copy())
