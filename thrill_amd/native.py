"""ctypes binding of libt9.so (include/thrill_amd.h).

Pointers are raw device addresses (torch tensor .data_ptr()); streams are
hipStream_t handles (torch.cuda.Stream.cuda_stream). No CPU fallback: a
missing library or GPU raises T9Error.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libt9.so")

u64 = ctypes.c_uint64
u32 = ctypes.c_uint32
i32 = ctypes.c_int
vp = ctypes.c_void_p


# t9_reduce_op / t9_val_type of include/thrill_amd.h
T9_OP_SUM, T9_OP_MIN, T9_OP_MAX = 0, 1, 2
T9_VAL_U64, T9_VAL_I64, T9_VAL_F64 = 0, 1, 2
T9_EINVAL = -22


class T9Error(RuntimeError):
    pass


def lib_path():
    return SO


def load_lib(path=None):
    path = path or SO
    if not os.path.exists(path):
        raise T9Error(
            f"libt9.so not found at {path}; build it with "
            "`make -C thrill_amd` (hipcc --offload-arch=gfx950). "
            "There is no CPU fallback.")
    return ctypes.CDLL(path)


_SIGS = {
    "t9_version": (ctypes.c_char_p, []),
    "t9_create": (i32, [ctypes.POINTER(vp), i32, i32, i32, vp]),
    "t9_destroy": (i32, [vp]),
    "t9_comm_id_size": (i32, []),
    "t9_comm_id": (i32, [vp]),
    "t9_comm_init": (i32, [vp, vp]),
    "t9_gen_u64": (i32, [vp, vp, u64, u64, u64, vp]),
    "t9_gen_records": (i32, [vp, vp, u64, u64, u64, vp]),
    "t9_sort_u64_workspace": (u64, [u64]),
    "t9_sort_u64": (i32, [vp, vp, u64, vp, vp]),
    "t9_sort_pairs_workspace": (u64, [u64]),
    "t9_sort_pairs_u64_u32": (i32, [vp, vp, vp, u64, vp, vp]),
    "t9_extract_key64": (i32, [vp, vp, u64, u32, u32, vp, vp, vp]),
    "t9_extract_key64_hist": (i32, [vp, vp, u64, u32, i32, vp, vp, vp, vp]),
    "t9_gather_records": (i32, [vp, vp, vp, u64, u32, vp, vp]),
    "t9_sort_records_workspace": (u64, [u64, u32]),
    "t9_sort_records": (i32, [vp, vp, vp, u64, u32, u32, vp, vp]),
    "t9_sort_records_keyle": (i32, [vp, vp, vp, u64, u32, vp, vp]),
    "t9_sort_last_schedule": (i32, [vp]),
    "t9_sort_last_tiecount": (i32, [vp]),
    "t9_sort_last_fused": (i32, [vp]),
    "t9_sort_last_packed": (i32, [vp]),
    "t9_extract_key64_le": (i32, [vp, vp, u64, u32, u32, vp, vp, vp]),
    "t9_classify_u64": (i32, [vp, vp, u64, u64, vp, vp, u32, vp, vp, vp]),
    "t9_classify_rec": (i32, [vp, vp, vp, u64, u64, vp, vp, vp, u32, u32,
                              vp, vp, vp]),
    "t9_partition_idx_workspace": (u64, [u64]),
    "t9_partition_idx": (i32, [vp, vp, u64, u32, vp, vp, vp, vp]),
    "t9_alltoall": (i32, [vp, vp, vp, vp, vp, vp, vp, u64, vp]),
    "t9_hash_bucket": (i32, [vp, vp, u64, u64, u32, vp, vp, vp]),
    "t9_reduce_by_index": (i32, [vp, vp, vp, u64, u64, u64, vp, vp, vp]),
    "t9_index_bucket": (i32, [vp, vp, u64, u64, u64, u32, vp, vp, vp, vp]),
    "t9_reduce_init": (i32, [vp, vp, u64, vp]),
    "t9_reduce_build": (i32, [vp, vp, vp, u64, vp, u64, u64, vp, vp]),
    "t9_reduce_drain": (i32, [vp, vp, u64, vp, vp, vp, vp]),
    "t9_reduce128_table_words": (u64, [u64]),
    "t9_reduce128_init": (i32, [vp, vp, u64, vp]),
    "t9_reduce128_build": (i32, [vp, vp, vp, vp, u64, vp, u64, u64, vp,
                                 vp]),
    "t9_reduce128_drain": (i32, [vp, vp, u64, vp, vp, vp, vp, vp]),
    "t9_reduce128_lookup": (i32, [vp, vp, vp, u64, vp, u64, u64, vp, vp]),
    "t9_hash2_of": (i32, [vp, vp, u64, vp, vp, vp]),
    "t9_reduce_init_op": (i32, [vp, vp, u64, i32, i32, vp]),
    "t9_reduce_build_op": (i32, [vp, vp, vp, u64, vp, u64, u64, i32, i32,
                                 vp, vp]),
    "t9_reduce_drain_op": (i32, [vp, vp, u64, i32, i32, vp, vp, vp, vp]),
    "t9_reduce128_init_op": (i32, [vp, vp, u64, i32, i32, vp]),
    "t9_reduce128_build_op": (i32, [vp, vp, vp, vp, u64, vp, u64, u64, i32,
                                    i32, vp, vp]),
    "t9_reduce128_drain_op": (i32, [vp, vp, u64, i32, i32, vp, vp, vp, vp,
                                    vp]),
    "t9_reduce_by_index_op_workspace": (u64, [u64]),
    "t9_reduce_by_index_op": (i32, [vp, vp, vp, u64, u64, u64, i32, i32,
                                    u64, vp, vp, vp, vp]),
    "t9_scan_geometry": (None, [ctypes.POINTER(u32), ctypes.POINTER(u32)]),
    "t9_scan_workspace": (u64, [u64]),
    "t9_scan_u64": (i32, [vp, vp, vp, u64, i32, i32, i32, u64, vp, vp, vp]),
    "t9_scan_kv": (i32, [vp, vp, vp, u64, i32, i32, u64, vp, vp, vp]),
    "t9_fold_u64": (i32, [vp, vp, u64, u32, i32, i32, vp, vp, vp]),
    "t9_join_geometry": (None, [ctypes.POINTER(u32), ctypes.POINTER(u32),
                                ctypes.POINTER(u32)]),
    "t9_join_workspace": (u64, [u64, u64]),
    "t9_join_count": (i32, [vp, vp, u64, vp, u64, ctypes.POINTER(u64), vp,
                            vp]),
    "t9_join_emit": (i32, [vp, u64, u64, vp, u64, vp, vp, vp]),
    "t9_text_tokenize_workspace": (u64, [u64]),
    "t9_text_tokenize": (i32, [vp, vp, u64, vp, vp, vp, vp, vp]),
    "t9_text_hash2": (i32, [vp, vp, u64, vp, vp, u64, vp, vp, vp, vp]),
    "t9_text_first_token": (i32, [vp, vp, u64, vp, u64, vp]),
    "t9_bucket_mod": (i32, [vp, vp, u64, u32, vp, vp, vp]),
    "t9_zipf_tokens": (i32, [vp, vp, vp, u64, u64, u64, u64, vp]),
    "t9_merge_u64": (i32, [vp, vp, u64, vp, u64, vp, vp]),
    "t9_merge_records": (i32, [vp, vp, u64, vp, u64, u32, vp, vp]),
    "t9_group_index_workspace": (u64, [u64]),
    "t9_group_index": (i32, [vp, vp, u64, vp, vp, vp, vp, vp]),
    "t9_perf_enable": (i32, [i32]),
    "t9_perf_read": (i32, [ctypes.c_char_p, ctypes.POINTER(ctypes.c_double),
                           ctypes.POINTER(u64)]),
    "t9_perf_reset": (i32, []),
}


class Native:
    """Loaded libt9 with a live t9_context. Requires a GPU."""

    def __init__(self, device=0, rank=0, world=1, comm=None):
        self._lib = load_lib()
        for name, (res, args) in _SIGS.items():
            fn = getattr(self._lib, name)
            fn.restype = res
            fn.argtypes = args
        ctx = vp()
        rc = self._lib.t9_create(ctypes.byref(ctx), device, rank, world,
                                 comm if comm else None)
        if rc != 0:
            raise T9Error(f"t9_create failed rc={rc} (no usable GPU?)")
        self.ctx = ctx

    def __getattr__(self, name):
        fn = getattr(self._lib, "t9_" + name, None)
        if fn is None:
            raise AttributeError(name)

        def call(*args):
            rc = fn(self.ctx, *args)
            if rc != 0:
                raise T9Error(f"t9_{name} failed rc={rc}")
            return rc
        return call

    # RCCL comm bootstrap (t9_comm_id takes no context argument)
    def comm_id(self):
        """rank 0: generate the ncclUniqueId as bytes."""
        size = self._lib.t9_comm_id_size()
        buf = (ctypes.c_uint8 * size)()
        rc = self._lib.t9_comm_id(buf)
        if rc != 0:
            raise T9Error(f"t9_comm_id failed rc={rc}")
        return bytes(buf)

    def comm_init(self, id_bytes):
        """every rank, collectively: connect the context's communicator."""
        buf = (ctypes.c_uint8 * len(id_bytes)).from_buffer_copy(id_bytes)
        rc = self._lib.t9_comm_init(self.ctx, buf)
        if rc != 0:
            raise T9Error(f"t9_comm_init failed rc={rc}")

    def sort_last_schedule(self):
        """0 = the last record sort ran serially; k > 0 = k chunks were
        gathered on the internal stream, overlapped with the sub sort."""
        k = self._lib.t9_sort_last_schedule(self.ctx)
        if k < 0:
            raise T9Error(f"t9_sort_last_schedule failed rc={k}")
        return k

    def sort_last_tiecount(self):
        """1 = the sub-bucket sort of the last record sort counted the
        equal-key neighbours itself; 0 = a standalone pass did."""
        k = self._lib.t9_sort_last_tiecount(self.ctx)
        if k < 0:
            raise T9Error(f"t9_sort_last_tiecount failed rc={k}")
        return k

    def sort_last_fused(self):
        """1 = the fused sort + gather kernel produced the output of the
        last record sort; 2 = it started but ties forced the redo; 0 = the
        sort and the gather ran as separate kernels."""
        k = self._lib.t9_sort_last_fused(self.ctx)
        if k < 0:
            raise T9Error(f"t9_sort_last_fused failed rc={k}")
        return k

    def sort_last_packed(self):
        """1 = the packed pass 2 + fused kernel produced the output of the
        last record sort; 2 = they started and the wide form redid it; 0 =
        not used."""
        k = self._lib.t9_sort_last_packed(self.ctx)
        if k < 0:
            raise T9Error(f"t9_sort_last_packed failed rc={k}")
        return k

    # perf registry functions take no context argument
    def perf_enable(self, on):
        self._lib.t9_perf_enable(1 if on else 0)

    def perf_read(self, cls):
        ms = ctypes.c_double()
        n = u64()
        rc = self._lib.t9_perf_read(cls.encode(), ctypes.byref(ms),
                                    ctypes.byref(n))
        if rc != 0:
            raise T9Error(f"t9_perf_read failed rc={rc}")
        return ms.value, n.value

    def perf_reset(self):
        self._lib.t9_perf_reset()

    def ws(self, name, *args):
        """workspace byte queries (no ctx argument)."""
        return getattr(self._lib, f"t9_{name}_workspace")(*args)

    def reduce128_table_words(self, capacity):
        """u64 elements of a 128-bit reduce table: 3 * capacity, or
        4 * capacity under T9_R128_STRIDE=4; no ctx argument, pure host
        code."""
        return self._lib.t9_reduce128_table_words(capacity)

    def scan_geometry(self):
        """(tile elements, tile totals per block of the middle pass) of
        the scan family; no ctx argument, pure host code."""
        t, p = u32(), u32()
        self._lib.t9_scan_geometry(ctypes.byref(t), ctypes.byref(p))
        return t.value, p.value

    def join_geometry(self):
        """(left keys per block of the bounds kernel, output positions per
        block of the emit kernel, most right keys a bounds block stages in
        LDS); no ctx argument, pure host code."""
        lt, ot, sk = u32(), u32(), u32()
        self._lib.t9_join_geometry(ctypes.byref(lt), ctypes.byref(ot),
                                   ctypes.byref(sk))
        return lt.value, ot.value, sk.value

    def join_count(self, d_lkeys, n_left, d_rkeys, n_right, d_ws, stream):
        """t9_join_count: match the two key arrays, leave the join state in
        d_ws and return the number of result pairs."""
        total = u64(0)
        rc = self._lib.t9_join_count(self.ctx, d_lkeys, n_left, d_rkeys,
                                     n_right, ctypes.byref(total), d_ws,
                                     stream)
        if rc != 0:
            raise T9Error(f"t9_join_count failed rc={rc}")
        return total.value

    def version(self):
        return self._lib.t9_version().decode()

    def close(self):
        if self.ctx:
            self._lib.t9_destroy(self.ctx)
            self.ctx = None
