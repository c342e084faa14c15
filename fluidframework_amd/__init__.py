"""fluidframework_amd -- MI355X replay / catch-up backend for Fluid Framework's merge-tree.

The hot path (Client.applyMsg over thousands of independent SharedString documents) runs in
hand-written HIP kernels (csrc/) behind the C ABI in include/mt_replay.h.  This Python
module is host plumbing mirroring the reference `Client` surface for tests and the bench;
the Node/N-API facade in js/ is the reference-language binding."""
import ctypes

import numpy as np

from . import _native
from .wire import CHECKSUM_DTYPE, OP_DTYPE, Batch, Interner  # noqa: F401

__all__ = ["MergeTreeBatch", "DeviceBatch", "Batch", "Interner", "DeltaLogOverflow"]


class DeltaLogOverflow(RuntimeError):
    """A document's delta log dropped records (mt_get_delta_log -> MT_E_OVERFLOW); `records`
    holds the whole records that were kept."""

    def __init__(self, msg, records):
        super().__init__(msg)
        self.records = records


def props_signature(pairs):
    """The device's 12-bit signature of a property set (mt_props_signature): pairs is a sequence
    of (key id, value id).  Needs the library, not a GPU."""
    a = np.ascontiguousarray(np.asarray(list(pairs), dtype=np.uint32).reshape(-1, 2))
    return int(_native.load().mt_props_signature(_native.ptr(a), a.shape[0]))


class PinnedArray:
    """A page-locked host buffer (mt_host_alloc) and its numpy view (`a`); the buffer is freed
    with this object, so keep it alive while the view is in use."""

    def __init__(self, lib, n, dtype):
        dt = np.dtype(dtype)
        nbytes = max(int(n), 1) * dt.itemsize
        self.lib = lib
        self.p = lib.mt_host_alloc(nbytes)
        if not self.p:
            raise MemoryError(f"mt_host_alloc({nbytes}) failed")
        self.a = np.frombuffer((ctypes.c_uint8 * nbytes).from_address(self.p), dtype=dt)

    def __del__(self):
        p, self.p = getattr(self, "p", None), None
        if p:
            try:
                self.lib.mt_host_free(p)
            except Exception:
                pass


class MergeTreeBatch:
    """N observer replicas (one per document) resident on one GPU.

    Mirrors, per document, `new Client(...)` + `startOrUpdateCollaboration` (MT/client.ts:
    75-84, 1053-1073), `applyMsg` (:797-819), `getLength` (:1051), `getText` via
    MergeTreeTextHelper (MT/textSegment.ts:154-172) and `getPropertiesAtPosition` (:1011-1025).
    """

    def __init__(self, n_docs, device=0, seg_capacity=0, block_capacity=0, heap_capacity=0,
                 text_capacity=0, props_capacity=0, delta_log_capacity=0, lds_seg_capacity=0,
                 page_capacity=0, page_heap_capacity=0, unsettled_capacity=0, uid_capacity=0,
                 lds_page_capacity=0, lds_unsettled_capacity=0, lds_page_heap_capacity=0, lds_narrow_overlap=0,
                 delta_log_mode=0, live_client=0, live_group_capacity=0, paged_slices=0, segment_ordinals=0,
                 overlap_arena_capacity=0):
        self.lib = _native.load()
        opt = _native.MtOptions(device, seg_capacity, block_capacity, heap_capacity,
                                text_capacity, props_capacity, delta_log_capacity,
                                lds_seg_capacity, page_capacity, page_heap_capacity,
                                unsettled_capacity, uid_capacity, lds_page_capacity,
                                lds_unsettled_capacity, lds_page_heap_capacity, lds_narrow_overlap,
                                delta_log_mode, live_client, live_group_capacity, paged_slices,
                                segment_ordinals, overlap_arena_capacity)
        self.h = self.lib.mt_create(n_docs, ctypes.byref(opt))
        if not self.h:
            raise RuntimeError("mt_create failed (no HIP device visible, or out of device memory)")
        self.n_docs = n_docs
        self.device = device

    def close(self):
        if self.h:
            self.lib.mt_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            msg = f"{what} failed ({rc}): {self.lib.mt_last_error(self.h).decode()}"
            raise RuntimeError(msg)

    # -------------------------------------------------------------- input
    def load_initial_text(self, seed_off, seed):
        seed_off = np.ascontiguousarray(seed_off, dtype=np.int64)
        seed = np.ascontiguousarray(seed, dtype=np.uint16)
        self._check(self.lib.mt_load_initial_text(self.h, _native.ptr(seed_off), _native.ptr(seed)),
                    "mt_load_initial_text")

    def start_collaboration(self, min_seq, cur_seq):
        """Client.startOrUpdateCollaboration(id, minSeq, currentSeq) for every document with
        min_seq[d] >= 0 (before its first message)."""
        ms = np.ascontiguousarray(min_seq, dtype=np.int32)
        cs = np.ascontiguousarray(cur_seq, dtype=np.int32)
        if ms.shape != (self.n_docs,) or cs.shape != (self.n_docs,):
            raise ValueError("start_collaboration: one minSeq and one currentSeq per document")
        self._check(self.lib.mt_start_collaboration(self.h, _native.ptr(ms), _native.ptr(cs)),
                    "mt_start_collaboration")

    def reset(self):
        """Asynchronously re-initialise every document from the loaded initial contents."""
        self._check(self.lib.mt_reset(self.h), "mt_reset")

    def apply_arrays(self, a):
        ops = np.ascontiguousarray(a["ops"], dtype=OP_DTYPE)
        off = np.ascontiguousarray(a["doc_off"], dtype=np.int64)
        text = np.ascontiguousarray(a["text"], dtype=np.uint16)
        props = np.ascontiguousarray(a["props"], dtype=np.uint32)
        self._check(self.lib.mt_apply_ops(self.h, _native.ptr(off), _native.ptr(ops), len(ops),
                                          _native.ptr(text), len(text), _native.ptr(props), len(props)),
                    "mt_apply_ops")

    @staticmethod
    def _snap_args(la):
        from .snapshot import SEG_DTYPE
        return [np.ascontiguousarray(la["doc_off"], dtype=np.int64), np.ascontiguousarray(la["n_header"], dtype=np.int32),
                np.ascontiguousarray(la["segs"], dtype=SEG_DTYPE), np.ascontiguousarray(la["text"], dtype=np.uint16),
                np.ascontiguousarray(la["props"], dtype=np.uint32), np.ascontiguousarray(la["min_seq"], dtype=np.int32),
                np.ascontiguousarray(la["cur_seq"], dtype=np.int32)]

    def load_snapshots(self, la):
        """Client.load of a decoded SnapshotV1 summary into every document
        (snapshot.SnapshotBatch.arrays(); MT/snapshotLoader.ts:36-228)."""
        off, nh, segs, text, props, mn, cu = self._snap_args(la)
        if len(off) != self.n_docs + 1:
            raise ValueError("one summary per document")
        self._check(self.lib.mt_load_snapshots(self.h, _native.ptr(off), _native.ptr(nh), _native.ptr(segs), len(segs),
                                               _native.ptr(text), len(text), _native.ptr(props), len(props),
                                               _native.ptr(mn), _native.ptr(cu)), "mt_load_snapshots")

    def load_summaries(self, summaries, interner, threads=8):
        """Client.load of every document from its summary blobs ({path: JSON text}, one dict
        per document): decoded on the host by the native decoder (snapdec, include/
        mt_snapshot.h; MT/snapshotLoader.ts:36-228), then loaded as load_snapshots does.
        Returns (catchup, clients): per document the legacy catch-up messages and the short
        client map its ops continue with (wire.Batch.add_doc(..., clients=...))."""
        import json as _json
        from .snapdec import SummaryDecoder
        la, catchup, clients = SummaryDecoder(interner, threads).decode(summaries)
        self.load_snapshots(la)
        return [_json.loads(c) if c is not None else [] for c in catchup], clients

    def upload_snapshots(self, la, doc_lo=0):
        """Device-resident summaries (mt_snapshots_upload); .load_async() enqueues a load.  With
        fewer summaries than documents, summary d is for document doc_lo + d
        (mt_snapshots_upload_range)."""
        off, nh, segs, text, props, mn, cu = self._snap_args(la)
        n = len(off) - 1
        s = self.lib.mt_snapshots_upload_range(self.h, doc_lo, n, _native.ptr(off), _native.ptr(nh), _native.ptr(segs),
                                               len(segs), _native.ptr(text), len(text), _native.ptr(props), len(props),
                                               _native.ptr(mn), _native.ptr(cu))
        if not s:
            raise RuntimeError(f"mt_snapshots_upload failed: {self.lib.mt_last_error(self.h).decode()}")
        return DeviceSnapshots(self, s)

    def catch_up(self, summaries, interner, threads=8, slice_docs=8192, packed=None):
        """Cold catch-up of every document from its summary blobs ({path: JSON text} per
        document; or `packed` = snapdec.SummaryDecoder.pack(summaries)), as load_summaries,
        in slices of `slice_docs` documents: the native decoder parses slice k + 1 on the
        host (a worker thread; the decoder's own threads inside) while slice k is uploaded
        and its load runs on the GPU (mt_snapshots_upload_range + mt_snapshots_load_async).
        Returns (catchup, clients) as load_summaries; the loads are enqueued on the handle's
        stream (sync() waits)."""
        import json as _json
        import queue
        import threading
        from .snapdec import SummaryDecoder
        paths, blobs, off = packed if packed is not None else SummaryDecoder.pack(summaries)
        if len(off) != self.n_docs + 1:
            raise ValueError("one summary per document")
        dec = SummaryDecoder(interner, threads)
        q = queue.Queue(maxsize=2)   # decoded slices waiting for their upload
        # arenas the decoder writes straight into, reused from slice to slice (and call to
        # call: no page faults once warm): three sets circulate -- one uploading, two decoded
        # or decoding.  (Page-locked arenas were measured slower: pinning costs more than the
        # ~17 GB/s pageable upload loses.)
        free_sets = queue.Queue()
        pool = getattr(self, "_catchup_arenas", None) or [{}, {}, {}]
        self._catchup_arenas = pool
        for ps in pool:
            free_sets.put(ps)

        stop = threading.Event()   # the consumer failed: the producer stops at its next slice

        def produce():
            try:
                for d0 in range(0, self.n_docs, slice_docs):
                    if stop.is_set():
                        return
                    d1 = min(self.n_docs, d0 + slice_docs)
                    b0, b1 = off[d0], off[d1]
                    sub = (paths[b0:b1], blobs[b0:b1], [o - b0 for o in off[d0:d1 + 1]])
                    pset = free_sets.get()

                    def alloc(m, dt, pset=pset):
                        key = np.dtype(dt).str
                        a = pset.get(key)
                        if a is None or len(a) < m:
                            a = np.empty(int(m * 1.25) + 64, dtype=dt)
                            pset[key] = a
                        return a[:m]
                    out, catchup, clients = dec.decode_packed_full(*sub, alloc=alloc)
                    q.put((d0, out, catchup, clients, pset))
                q.put(None)
            except BaseException as e:   # surfaces in the consumer
                q.put(e)

        t = threading.Thread(target=produce, daemon=True)
        t.start()
        from .snapdec import ClientMaps
        catchup_all, clients_all, held = [], ClientMaps([]), []
        try:
            while True:
                item = q.get()
                if item is None:
                    break
                if isinstance(item, BaseException):
                    raise item
                d0, out, catchup, clients, pset = item
                snaps = self.upload_snapshots(out, doc_lo=d0)   # synchronous copies: the set is free again
                free_sets.put(pset)
                snaps.load_async()
                held.append(snaps)   # device copies stay alive until the loads have run
                cu_msgs = [[] for _ in catchup]
                for i, c in enumerate(catchup):
                    if c is not None:
                        cu_msgs[i] = _json.loads(c)
                catchup_all += cu_msgs
                clients_all = clients_all + clients
        finally:
            # on any exit: unblock and join the producer (it may wait for a free arena set or
            # on the queue), finish the enqueued loads, free every uploaded snapshot set
            stop.set()
            while t.is_alive():
                try:
                    item = q.get(timeout=0.05)
                    if isinstance(item, tuple):
                        free_sets.put(item[4])
                except queue.Empty:
                    pass
                free_sets.put({})
            t.join()
            try:
                self.sync()
            finally:
                for s_ in held:
                    s_.free()
        return catchup_all, clients_all

    def ingest_logs(self, slices, interner=None, threads=8, pinned=True):
        """Sequenced message logs in, replayed documents out, as a pipeline (SEQ/sequence.ts:579-616
        feeds SharedSegmentSequence JSON messages): ``slices`` yields (d0, blobs) -- the JSON
        message arrays of documents [d0, d0 + len(blobs)), in document order.  A host thread
        encodes slice k + 1 (the native encoder, mt_opdec, its own threads inside) while this
        thread uploads slice k (mt_batch_upload) and enqueues its replay on the handle's
        stream, behind slice k - 1's (mt_batch_apply_async).  Arenas are reused from slice to
        slice, and so is the encoder (its buffers stay warm from call to call for the same
        interner and thread count); with `pinned` the arenas are page-locked (mt_host_alloc),
        so the upload is a DMA that takes no host core from the encoder.  Returns the seconds each stage was busy: {"encode",
        "upload", "apply_wait", "wall"} (apply_wait: time the caller's thread waited for the
        previous slice's replay) and "encode_slices", each slice's encode seconds."""
        import queue
        import threading
        import time as _time
        from .opdec import MessageDecoder
        interner = interner or getattr(self, "_ingest_interner", None) or Interner(synthetic=True)
        self._ingest_interner = interner
        dec = getattr(self, "_ingest_dec", None)
        if dec is None or dec.interner is not interner or dec.threads != threads:
            dec = self._ingest_dec = MessageDecoder(interner, threads=threads)
        q = queue.Queue(maxsize=1)                     # one encoded slice waiting for its upload
        free_sets = queue.Queue()
        for ps in getattr(self, "_ingest_arenas", None) or [{}, {}]:
            free_sets.put(ps)
        stop = threading.Event()
        busy = {"encode": 0.0, "upload": 0.0, "apply_wait": 0.0, "encode_slices": []}

        def produce():
            try:
                for d0, blobs in slices:
                    if stop.is_set():
                        return
                    pset = free_sets.get()
                    if stop.is_set():
                        return

                    def alloc(m, dt, pset=pset):
                        key = np.dtype(dt).str
                        a = pset.get(key)
                        if a is None or len(a) < m:
                            n = int(m * 1.25) + 64
                            if pinned:
                                pset["pin" + key] = PinnedArray(self.lib, n, dt)
                                a = pset["pin" + key].a
                            else:
                                a = np.empty(n, dtype=dt)
                            pset[key] = a
                        return a[:m]
                    t = _time.perf_counter()
                    off = pset.setdefault("off", np.zeros(self.n_docs + 1, dtype=np.int64))
                    n = len(blobs)
                    sub = np.zeros(n + 1, dtype=np.int64)
                    out = dec.decode_packed(blobs, alloc=alloc, doc_off_out=sub)
                    dec.remap(out)
                    off[: d0 + 1] = 0
                    off[d0 + 1: d0 + n + 1] = sub[1:]
                    off[d0 + n + 1:] = sub[-1]
                    out["doc_off"] = off
                    busy["encode_slices"].append(_time.perf_counter() - t)
                    busy["encode"] += busy["encode_slices"][-1]
                    q.put((out, pset))
                q.put(None)
            except BaseException as e:   # surfaces in the consumer
                q.put(e)

        t_wall = _time.perf_counter()
        th = threading.Thread(target=produce, daemon=True)
        th.start()
        prev = None
        try:
            while True:
                item = q.get()
                if item is None:
                    break
                if isinstance(item, BaseException):
                    raise item
                out, pset = item
                t = _time.perf_counter()
                b = self.upload(out)   # (validation + copies: the arena set is free again after)
                busy["upload"] += _time.perf_counter() - t
                free_sets.put(pset)
                if prev is not None:
                    # before this slice's replay is queued: hipFree waits for the device to go
                    # idle, and slice k - 1's replay has ended while slice k was encoded, so
                    # nothing waits here (after the enqueue it would wait -- spinning a host
                    # core the encoder needs -- for slice k's whole replay)
                    t = _time.perf_counter()
                    prev.free()
                    busy["apply_wait"] += _time.perf_counter() - t
                t = _time.perf_counter()
                b.apply_async()        # (waits for the previous slice's replay and growth step)
                busy["apply_wait"] += _time.perf_counter() - t
                prev = b
            self.sync()
        finally:
            stop.set()
            while th.is_alive():
                try:
                    item = q.get(timeout=0.05)
                    if isinstance(item, tuple):
                        free_sets.put(item[1])
                except queue.Empty:
                    pass
                free_sets.put({})
            th.join()
            if prev is not None:
                self.sync()
                prev.free()
            self._ingest_arenas = []
            while not free_sets.empty():
                ps = free_sets.get()
                if ps:
                    self._ingest_arenas.append(ps)
        busy["wall"] = _time.perf_counter() - t_wall
        return busy

    def extract_snapshots_raw(self):
        """mt_extract_snapshots as concatenated arrays: (counts[n_docs, 3], records, text,
        props, min_seq, cur_seq); record offsets are relative to their document's arenas."""
        from .snapshot import SEG_DTYPE
        io = np.zeros(3 * self.n_docs, dtype=np.int64)
        self._check(self.lib.mt_extract_snapshots(self.h, _native.ptr(io), None, None, None, None, None),
                    "mt_extract_snapshots")
        tot = io.reshape(-1, 3).sum(axis=0)
        recs = np.zeros(max(int(tot[0]), 1), dtype=SEG_DTYPE)
        text = np.zeros(max(int(tot[1]), 1), dtype=np.uint16)
        props = np.zeros(max(int(tot[2]), 1), dtype=np.uint32)
        mn = np.zeros(self.n_docs, dtype=np.int32)
        cu = np.zeros(self.n_docs, dtype=np.int32)
        self._check(self.lib.mt_extract_snapshots(self.h, _native.ptr(io), _native.ptr(recs), _native.ptr(text),
                                                  _native.ptr(props), _native.ptr(mn), _native.ptr(cu)),
                    "mt_extract_snapshots")
        return io.reshape(-1, 3), recs[: int(tot[0])], text, props, mn, cu

    def extract_snapshots(self):
        """SnapshotV1.extractSync of every document (mt_extract_snapshots): per document
        (records, text, props, min_seq, cur_seq); records index that document's arenas."""
        from .snapshot import SEG_DTYPE
        io = np.zeros(3 * self.n_docs, dtype=np.int64)
        self._check(self.lib.mt_extract_snapshots(self.h, _native.ptr(io), None, None, None, None, None),
                    "mt_extract_snapshots")
        tot = io.reshape(-1, 3).sum(axis=0)
        recs = np.zeros(max(int(tot[0]), 1), dtype=SEG_DTYPE)
        text = np.zeros(max(int(tot[1]), 1), dtype=np.uint16)
        props = np.zeros(max(int(tot[2]), 1), dtype=np.uint32)
        mn = np.zeros(self.n_docs, dtype=np.int32)
        cu = np.zeros(self.n_docs, dtype=np.int32)
        self._check(self.lib.mt_extract_snapshots(self.h, _native.ptr(io), _native.ptr(recs), _native.ptr(text),
                                                  _native.ptr(props), _native.ptr(mn), _native.ptr(cu)),
                    "mt_extract_snapshots")
        out = []
        c = io.reshape(-1, 3)
        r0 = t0 = p0 = 0
        for d in range(self.n_docs):
            nr, nt, np_ = (int(x) for x in c[d])
            out.append(dict(segs=recs[r0:r0 + nr], text=text[t0:t0 + nt], props=props[p0:p0 + np_],
                            min_seq=int(mn[d]), cur_seq=int(cu[d])))
            r0, t0, p0 = r0 + nr, t0 + nt, p0 + np_
        return out

    def upload(self, a):
        return DeviceBatch(self, a)

    def generate(self, cfg, doc_base=0, trace=None, ops_per_doc=None, doc_ids=None):
        """Device-generated batch (mt_generate); ops_per_doc: a length per document, doc_ids:
        their global indices (mt_generate_docs), else cfg["ops"] each and doc_base + d."""
        c = _native.gen_cfg(cfg)
        if ops_per_doc is not None or doc_ids is not None:
            lens = None if ops_per_doc is None else np.ascontiguousarray(ops_per_doc, dtype=np.int32)
            ids = None if doc_ids is None else np.ascontiguousarray(doc_ids, dtype=np.int32)
            for x in (lens, ids):
                if x is not None and x.shape != (self.n_docs,):
                    raise ValueError("ops_per_doc / doc_ids: one per document")
            b = self.lib.mt_generate_docs(self.h, ctypes.byref(c), doc_base, _native.ptr(lens), _native.ptr(ids),
                                          _native.ptr(trace))
        else:
            b = self.lib.mt_generate(self.h, ctypes.byref(c), doc_base, _native.ptr(trace))
        if not b:
            raise RuntimeError(f"mt_generate failed: {self.lib.mt_last_error(self.h).decode()}")
        return DeviceBatch(self, None, handle=b)

    def generated_seeds(self, cfg, doc_base=0, doc_ids=None):
        c = _native.gen_cfg(cfg)
        ids = None if doc_ids is None else np.ascontiguousarray(doc_ids, dtype=np.int32)
        off = np.zeros(self.n_docs + 1, dtype=np.int64)
        self._check(self.lib.mt_generated_seeds_docs(self.h, ctypes.byref(c), doc_base, _native.ptr(ids),
                                                     _native.ptr(off), None), "mt_generated_seeds")
        seed = np.zeros(max(int(off[-1]), 1), dtype=np.uint16)
        self._check(self.lib.mt_generated_seeds_docs(self.h, ctypes.byref(c), doc_base, _native.ptr(ids),
                                                     _native.ptr(off), _native.ptr(seed)), "mt_generated_seeds")
        return off, seed

    def sync(self):
        self._check(self.lib.mt_sync(self.h), "mt_sync")

    def last_hbm_docs(self):
        """Documents of the last batch replayed from HBM (outgrew the LDS tier)."""
        out = np.zeros(8, dtype=np.uint32)
        self._check(self.lib.mt_last_hbm_docs(self.h, _native.ptr(out)), "mt_last_hbm_docs")
        return dict(total=int(out[0]), spilled=int(out[1]), segments=int(out[2]), blocks=int(out[3]), heap=int(out[4]),
                    text=int(out[5]), props=int(out[6]), at_load=int(out[7]))

    def last_paged_peaks(self):
        """High-water marks of the paged documents of the last batch / generation."""
        out = np.zeros(5, dtype=np.uint32)
        self._check(self.lib.mt_last_paged_peaks(self.h, _native.ptr(out)), "mt_last_paged_peaks")
        return dict(pages=int(out[0]), unsettled=int(out[1]), heap=int(out[2]), segments=int(out[3]),
                    tight_handovers=int(out[4]))

    def last_zamboni(self):
        """Zamboni's scours of the last batch / generation outside the staged page: done in place
        on the page in HBM, or through the window after all (mt_last_zamboni); in_place_packs:
        those of in_place that repacked the page's leaf blocks as well (mt_last_zamboni_packs)."""
        out = np.zeros(2, dtype=np.uint32)
        self._check(self.lib.mt_last_zamboni(self.h, _native.ptr(out)), "mt_last_zamboni")
        packs = np.zeros(1, dtype=np.uint32)
        self._check(self.lib.mt_last_zamboni_packs(self.h, _native.ptr(packs)), "mt_last_zamboni_packs")
        return {"in_place": int(out[0]), "fallback": int(out[1]), "in_place_packs": int(packs[0])}

    def last_range_paths(self):
        """The last batch's / generation's remove and annotate messages on paged documents by
        path (mt_last_range_paths): one_page took the single-page path to its end, split_fallback
        entered it and left it for a pending page split, general went the general way from the start."""
        out = np.zeros(3, dtype=np.uint32)
        self._check(self.lib.mt_last_range_paths(self.h, _native.ptr(out)), "mt_last_range_paths")
        return {"one_page": int(out[0]), "split_fallback": int(out[1]), "general": int(out[2])}

    def last_grown(self):
        """The last batch's growth step (mt_last_grown): documents moved to larger paged
        capacities, rounds, documents in the big region and its capacities."""
        out = np.zeros(6, dtype=np.uint32)
        self._check(self.lib.mt_last_grown(self.h, _native.ptr(out)), "mt_last_grown")
        return dict(zip(["grown", "rounds", "in_big_region", "pages", "unsettled", "heap"], (int(x) for x in out)))

    def last_kernel_ms(self):
        return float(self.lib.mt_last_kernel_ms(self.h))

    def set_stream_priority(self, priority):
        """mt_set_stream_priority: > 0 the device's highest stream priority, < 0 its lowest."""
        self._check(self.lib.mt_set_stream_priority(self.h, int(priority)), "mt_set_stream_priority")

    def last_load_ms(self):
        """Device time of the most recent snapshot load's kernels (mt_last_load_ms)."""
        return float(self.lib.mt_last_load_ms(self.h))

    # -------------------------------------------------------------- read-out
    def status(self):
        out = np.zeros(self.n_docs, dtype=np.int32)
        self._check(self.lib.mt_get_status(self.h, _native.ptr(out)), "mt_get_status")
        return out

    def get_length(self, doc):
        out = ctypes.c_uint32()
        self._check(self.lib.mt_get_length(self.h, doc, ctypes.byref(out)), "mt_get_length")
        return out.value

    def get_text(self, doc):
        n = ctypes.c_uint32()
        self._check(self.lib.mt_get_text(self.h, doc, None, 0, ctypes.byref(n)), "mt_get_text")
        buf = np.zeros(max(n.value, 1), dtype=np.uint16)
        self._check(self.lib.mt_get_text(self.h, doc, _native.ptr(buf), n.value, ctypes.byref(n)),
                    "mt_get_text")
        return buf[: n.value].tobytes().decode("utf-16-le", errors="surrogatepass")

    # bulk / ranged text (mt_get_texts): SharedString.getText(start, end), getTextWithPlaceholders
    # and getTextRangeWithPlaceholders (sharedString.ts:222-236) for many documents in one launch
    def _text_queries(self, docs, start, end, placeholder):
        """(n, docs, start, end, marker_unit) as mt_get_texts takes them; scalars broadcast."""
        if isinstance(placeholder, str):
            units = np.frombuffer(placeholder.encode("utf-16-le", errors="surrogatepass"), dtype=np.uint16)
            if len(units) > 1:
                raise ValueError("get_texts: the placeholder is empty or one UTF-16 unit")
            placeholder = int(units[0]) if len(units) else 0
        if docs is not None:
            docs = np.ascontiguousarray(docs, dtype=np.uint32).reshape(-1)
        n = len(docs) if docs is not None else self.n_docs
        if start is not None:
            start = np.ascontiguousarray(np.broadcast_to(np.asarray(start, dtype=np.int32), (n,)))
        if end is not None:
            end = np.asarray([-1 if e is None else e for e in end] if isinstance(end, (list, tuple)) else end)
            end = np.ascontiguousarray(np.broadcast_to(end.astype(np.int32), (n,)))
        return n, docs, start, end, int(placeholder)

    def get_texts_raw(self, docs=None, start=None, end=None, placeholder=""):
        """(off, units): query q's UTF-16 units are units[off[q]:off[q + 1]]."""
        n, docs, start, end, mu = self._text_queries(docs, start, end, placeholder)
        off = np.zeros(n + 1, dtype=np.int64)
        args = (self.h, n, _native.ptr(docs), _native.ptr(start), _native.ptr(end), mu, _native.ptr(off))
        self._check(self.lib.mt_get_texts(*args, None, 0), "mt_get_texts")
        units = np.zeros(max(int(off[n]), 1), dtype=np.uint16)
        self._check(self.lib.mt_get_texts(*args, _native.ptr(units), int(off[n])), "mt_get_texts")
        return off, units[: int(off[n])]

    def get_texts(self, docs=None, start=None, end=None, placeholder=""):
        """The observer-view text of each query (doc, start, end): every document when docs is
        None, whole documents when start / end are None (an end of -1 or None: the document's
        length).  start and end are clamped into [0, length].  placeholder "": markers give
        nothing; one UTF-16 unit (" " in getTextWithPlaceholders): each marker gives that unit."""
        off, units = self.get_texts_raw(docs, start, end, placeholder)
        raw = units.tobytes()
        return [raw[2 * int(off[q]): 2 * int(off[q + 1])].decode("utf-16-le", errors="surrogatepass")
                for q in range(len(off) - 1)]

    def get_texts_device(self, docs=None, start=None, end=None, placeholder="", out=None):
        """get_texts_raw with the results left on the handle's device: (off, units) torch tensors
        (int64 [n + 1], int16 holding the UTF-16 units).  out: an int16 tensor on that device to
        fill (at least the result's size); units is then its leading slice.  (A process that
        uses torch on the GPU imports it before it creates its first handle, as bench.py does:
        the replay library then shares torch's HIP runtime.)"""
        import torch
        n, docs, start, end, mu = self._text_queries(docs, start, end, placeholder)
        dev = torch.device("cuda", self.device)
        off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        args = (self.h, n, _native.ptr(docs), _native.ptr(start), _native.ptr(end), mu, ctypes.c_void_p(off.data_ptr()))
        if out is None:
            self._check(self.lib.mt_get_texts_device(*args, None, 0), "mt_get_texts_device")
            out = torch.empty(max(int(off[n]), 1), dtype=torch.int16, device=dev)
        elif out.dtype != torch.int16 or out.device != dev or not out.is_contiguous():
            raise ValueError("get_texts_device: out is a contiguous int16 tensor on the handle's device")
        self._check(self.lib.mt_get_texts_device(*args, ctypes.c_void_p(out.data_ptr()), out.numel()),
                    "mt_get_texts_device")
        return off, out[: int(off[n])]

    def last_text_ms(self):
        """Device time (ms) of the last get_texts call's counting pass and gather."""
        out = np.zeros(2, dtype=np.float32)
        self._check(self.lib.mt_last_text_ms(self.h, _native.ptr(out)), "mt_last_text_ms")
        return float(out[0]), float(out[1])

    def get_segments(self, doc):
        nr, nl = ctypes.c_uint32(), ctypes.c_uint32()
        self._check(self.lib.mt_get_segments(self.h, doc, None, 0, ctypes.byref(nr), None, 0,
                                             ctypes.byref(nl)), "mt_get_segments")
        rows = np.zeros((max(nr.value, 1), 8), dtype=np.int32)
        leaves = np.zeros(max(nl.value, 1), dtype=np.int32)
        self._check(self.lib.mt_get_segments(self.h, doc, _native.ptr(rows), nr.value, ctypes.byref(nr),
                                             _native.ptr(leaves), nl.value, ctypes.byref(nl)),
                    "mt_get_segments")
        return rows[: nr.value], leaves[: nl.value].tolist()

    def get_overlap_arena(self, doc):
        """A paged document's overflow overlap arena (mt_get_overlap_arena)."""
        out = np.zeros(7, dtype=np.int32)
        self._check(self.lib.mt_get_overlap_arena(self.h, doc, _native.ptr(out)), "mt_get_overlap_arena")
        return dict(zip(["capacity", "fill", "half", "largest_set", "live_units", "made", "peak_fill"],
                        (int(x) for x in out)))

    def get_segment_props(self, doc, i):
        pairs = np.zeros(64, dtype=np.uint32)
        n = ctypes.c_int32()
        self._check(self.lib.mt_get_segment_props(self.h, doc, i, _native.ptr(pairs), 32, ctypes.byref(n)),
                    "mt_get_segment_props")
        if n.value < 0:
            return None
        return [(int(pairs[2 * j]), int(pairs[2 * j + 1])) for j in range(n.value)]

    def get_all_segment_props(self, doc):
        """get_segment_props of every segment, from one copy of the document."""
        n = ctypes.c_uint64()
        self._check(self.lib.mt_get_all_segment_props(self.h, doc, None, 0, ctypes.byref(n)), "mt_get_all_segment_props")
        buf = np.zeros(max(n.value, 1), dtype=np.int32)
        self._check(self.lib.mt_get_all_segment_props(self.h, doc, _native.ptr(buf), n.value, ctypes.byref(n)),
                    "mt_get_all_segment_props")
        out, w, b = [], 0, buf.tolist()
        while w < n.value:
            k = b[w]
            w += 1
            if k < 0:
                out.append(None)
                continue
            out.append([(b[w + 2 * j] & 0xFFFFFFFF, b[w + 2 * j + 1] & 0xFFFFFFFF) for j in range(k)])
            w += 2 * k
        return out

    # -------------------------------------------------------------- segment read-outs
    @staticmethod
    def _seg_info(info, text):
        if info.row < 0:
            return None
        out = dict(row=info.row, uid=info.uid, position=info.position, offset=info.offset, length=info.length,
                   seq=info.seq, client=info.client, removed_seq=info.removed_seq,
                   removed_client=info.removed_client, marker_ref_type=info.marker_ref_type,
                   ordinal=list(info.ordinal[:info.ordinal_len]) if info.ordinal_len >= 0 else None)
        if info.marker_ref_type < 0:
            out["text"] = text[:info.text_len].tobytes().decode("utf-16-le", errors="surrogatepass")
        return out

    def get_containing_segment(self, doc, pos, ref_seq=0, client=0, text_cap=1 << 16):
        """MergeTree.getContainingSegment(pos, refSeq, clientId) (MT/mergeTree.ts:1656-1667):
        the segment's read-out (dict) with `offset` = pos - its position, or None."""
        info = _native.MtSegInfo()
        text = np.zeros(text_cap, dtype=np.uint16)
        self._check(self.lib.mt_get_containing_segment(self.h, doc, pos, ref_seq, client, ctypes.byref(info),
                                                       _native.ptr(text), text_cap), "mt_get_containing_segment")
        return self._seg_info(info, text)

    def get_segment_by_uid(self, doc, uid, ref_seq=0, client=0, text_cap=1 << 16):
        """MergeTree.getPosition(segment, refSeq, clientId) (:1619-1636) of segment `uid` as
        the read-out's `position`; None once it left the tree."""
        info = _native.MtSegInfo()
        text = np.zeros(text_cap, dtype=np.uint16)
        self._check(self.lib.mt_get_segment_by_uid(self.h, doc, uid, ref_seq, client, ctypes.byref(info),
                                                   _native.ptr(text), text_cap), "mt_get_segment_by_uid")
        return self._seg_info(info, text)

    def get_view_lengths(self, docs, ref_seq, client):
        """MergeTree.getLength(refSeq, clientId) (:1610-1612) for each (doc, refSeq, client):
        the root's partial length in a remote view (every refSeq of the collab window,
        MT/partialLengths.ts:455-486), the local length for client 0."""
        docs = np.ascontiguousarray(docs, dtype=np.uint32)
        ref = np.ascontiguousarray(ref_seq, dtype=np.int32)
        cli = np.ascontiguousarray(client, dtype=np.int32)
        out = np.zeros(len(docs), dtype=np.int32)
        self._check(self.lib.mt_get_view_lengths(self.h, len(docs), _native.ptr(docs), _native.ptr(ref),
                                                 _native.ptr(cli), _native.ptr(out)), "mt_get_view_lengths")
        return out

    # bulk segment read-outs (mt_locate_segments / mt_locate_uids / mt_get_view_lengths_bulk /
    # mt_resolve_remote_positions): the three calls above for many cursors in one launch
    def _cursor_queries(self, docs, key, ref_seq, client, key_dtype):
        """(n, docs, key, ref_seq, client) as mt_locate_* take them; scalars broadcast; ref_seq /
        client None: the observer view for every query."""
        if docs is not None:
            docs = np.ascontiguousarray(docs, dtype=np.uint32).reshape(-1)
        n = len(docs) if docs is not None else self.n_docs
        if key is not None:
            key = np.ascontiguousarray(np.broadcast_to(np.asarray(key, dtype=key_dtype), (n,)))
        if client is None:
            ref_seq = None
        else:
            client = np.ascontiguousarray(np.broadcast_to(np.asarray(client, dtype=np.int32), (n,)))
            ref_seq = np.ascontiguousarray(np.broadcast_to(np.asarray(0 if ref_seq is None else ref_seq,
                                                                      dtype=np.int32), (n,)))
        return n, docs, key, ref_seq, client

    def locate_segments(self, docs, pos, ref_seq=None, client=None):
        """MergeTree.getContainingSegment(pos, refSeq, clientId) for each (doc, pos, refSeq,
        client): a structured array of mt_seg_hit records (_native.SEG_HIT_DTYPE; row -1: no
        segment; `local_position`: the segment's position in the observer view)."""
        n, docs, pos, ref, cli = self._cursor_queries(docs, pos, ref_seq, client, np.int32)
        out = np.zeros(n, dtype=_native.SEG_HIT_DTYPE)
        self._check(self.lib.mt_locate_segments(self.h, n, _native.ptr(docs), _native.ptr(pos), _native.ptr(ref),
                                                _native.ptr(cli), _native.ptr(out)), "mt_locate_segments")
        return out

    def locate_uids(self, docs, uids, ref_seq=None, client=None):
        """MergeTree.getPosition(segment, refSeq, clientId) of the segments with ids `uids`, as
        locate_segments' records (offset 0; row -1 once a segment left the tree)."""
        n, docs, uids, ref, cli = self._cursor_queries(docs, uids, ref_seq, client, np.uint32)
        out = np.zeros(n, dtype=_native.SEG_HIT_DTYPE)
        self._check(self.lib.mt_locate_uids(self.h, n, _native.ptr(docs), _native.ptr(uids), _native.ptr(ref),
                                            _native.ptr(cli), _native.ptr(out)), "mt_locate_uids")
        return out

    def locate_segments_device(self, docs, pos=None, ref_seq=None, client=None, uids=None):
        """locate_segments (or, with uids, locate_uids) with the records left on the handle's
        device: an int32 torch tensor [n, 12], the words of mt_seg_hit in order (torch is imported
        before the first handle is created, as for get_texts_device)."""
        import torch
        by_uid = uids is not None
        n, docs, key, ref, cli = self._cursor_queries(docs, uids if by_uid else pos, ref_seq, client,
                                                      np.uint32 if by_uid else np.int32)
        out = torch.empty((n, _native.SEG_HIT_DTYPE.itemsize // 4), dtype=torch.int32,
                          device=torch.device("cuda", self.device))
        fn, name = ((self.lib.mt_locate_uids_device, "mt_locate_uids_device") if by_uid
                    else (self.lib.mt_locate_segments_device, "mt_locate_segments_device"))
        self._check(fn(self.h, n, _native.ptr(docs), _native.ptr(key), _native.ptr(ref), _native.ptr(cli),
                       ctypes.c_void_p(out.data_ptr())), name)
        return out

    def get_view_lengths_bulk(self, docs, ref_seq=None, client=None):
        """get_view_lengths summed on the device, one launch for all queries."""
        n, docs, _, ref, cli = self._cursor_queries(docs, None, ref_seq, client, np.int32)
        out = np.zeros(n, dtype=np.int32)
        self._check(self.lib.mt_get_view_lengths_bulk(self.h, n, _native.ptr(docs), _native.ptr(ref), _native.ptr(cli),
                                                      _native.ptr(out)), "mt_get_view_lengths_bulk")
        return out

    def resolve_remote_positions(self, docs, pos, ref_seq, client):
        """MergeTree.resolveRemoteClientPosition(pos, refSeq, clientId) (MT/mergeTree.ts:2140-2160)
        for each query: the position in the observer view, -1 where the reference returns
        undefined."""
        n, docs, pos, ref, cli = self._cursor_queries(docs, pos, ref_seq, client, np.int32)
        out = np.zeros(n, dtype=np.int32)
        self._check(self.lib.mt_resolve_remote_positions(self.h, n, _native.ptr(docs), _native.ptr(pos),
                                                         _native.ptr(ref), _native.ptr(cli), _native.ptr(out)),
                    "mt_resolve_remote_positions")
        return out

    def last_locate(self):
        """(queries, of them answered by the host path, kernel ms) of the last bulk segment
        read-out."""
        out = np.zeros(2, dtype=np.int64)
        ms = ctypes.c_float()
        self._check(self.lib.mt_last_locate(self.h, _native.ptr(out), ctypes.byref(ms)), "mt_last_locate")
        return int(out[0]), int(out[1]), float(ms.value)

    # bulk marker queries (mt_find_tiles / mt_find_markers_by_id): SharedString.findTile and
    # getMarkerFromId for many queries in one launch, in the replica's own view
    TILE_LABELS_KEY, MARKER_ID_KEY = "referenceTileLabels", "markerId"

    def _label_ids(self, interner, label):
        """Ids (ascending, without flag bits) of the interned values that yield `label` when
        JavaScript iterates them: lists holding it, strings holding it as a character.  Kept per
        label and extended when the interner has grown."""
        cache = getattr(self, "_tile_labels", None)
        if cache is None or cache[0] is not interner:
            cache = self._tile_labels = (interner, {})
        seen, ids = cache[1].setdefault(label, [0, []])
        vals = interner.vals
        for i in range(seen, len(vals)):
            v = vals[i]
            if (isinstance(v, list) and any(isinstance(x, str) and x == label for x in v)) or \
                    (isinstance(v, str) and len(label) == 1 and label in v):
                ids.append(i)
        cache[1][label][0] = len(vals)
        return ids

    def _tile_queries(self, docs, pos, labels, preceding, interner):
        if interner is None:
            raise ValueError("find_tiles: pass the interner the batches were encoded with")
        if docs is not None:
            docs = np.ascontiguousarray(docs, dtype=np.uint32).reshape(-1)
        n = len(docs) if docs is not None else self.n_docs
        if pos is None or np.isscalar(pos):
            pos = np.full(n, -1 if pos is None else int(pos), dtype=np.int32)
        elif isinstance(pos, np.ndarray) and pos.dtype.kind in "iu":
            pos = np.ascontiguousarray(pos, dtype=np.int32).reshape(-1)
        else:
            pos = np.ascontiguousarray([-1 if p is None else int(p) for p in pos], dtype=np.int32)
        if len(pos) != n:
            raise ValueError("find_tiles: one position per query")
        one = isinstance(labels, str)
        names = [labels] if one else sorted(set(labels))
        if not one and len(labels) != n:
            raise ValueError("find_tiles: one label per query")
        index = {s: i for i, s in enumerate(names)}
        sets = [self._label_ids(interner, s) for s in names]
        off = np.zeros(len(names) + 1, dtype=np.uint32)
        off[1:] = np.cumsum([len(s) for s in sets])
        vals = np.ascontiguousarray([i for s in sets for i in s], dtype=np.uint32)
        label = np.zeros(n, dtype=np.uint32) if one else np.ascontiguousarray([index[s] for s in labels], dtype=np.uint32)
        prec = np.ascontiguousarray(np.broadcast_to(np.asarray(preceding, dtype=bool), (n,)), dtype=np.uint8)
        # a key the interner has never seen is held by no record
        key = 0xFFFFFFFF if interner.synthetic else interner.key_ids.get(self.TILE_LABELS_KEY, 0xFFFFFFFF)
        return n, docs, pos, prec, label, key, len(names), off, vals

    def find_tiles(self, docs, pos, labels, preceding=True, interner=None):
        """SharedString.findTile(pos, label, preceding) for each (doc, pos, label, preceding):
        mt_seg_hit records (_native.SEG_HIT_DTYPE) of the nearest tile marker carrying the label
        at or before (preceding) / at or after the position; row -1: none; `position` is the
        marker's.  pos entries may be None (undefined); labels: one string, or one per query;
        preceding: one flag, or one per query."""
        n, docs, pos, prec, label, key, nl, off, vals = self._tile_queries(docs, pos, labels, preceding, interner)
        out = np.zeros(n, dtype=_native.SEG_HIT_DTYPE)
        self._check(self.lib.mt_find_tiles(self.h, n, _native.ptr(docs), _native.ptr(pos), _native.ptr(prec),
                                           _native.ptr(label), key, nl, _native.ptr(off), _native.ptr(vals),
                                           _native.ptr(out)), "mt_find_tiles")
        return out

    def find_tiles_device(self, docs, pos, labels, preceding=True, interner=None):
        """find_tiles with the records left on the handle's device: an int32 torch tensor [n, 12]
        (as locate_segments_device)."""
        import torch
        n, docs, pos, prec, label, key, nl, off, vals = self._tile_queries(docs, pos, labels, preceding, interner)
        out = torch.empty((n, _native.SEG_HIT_DTYPE.itemsize // 4), dtype=torch.int32,
                          device=torch.device("cuda", self.device))
        self._check(self.lib.mt_find_tiles_device(self.h, n, _native.ptr(docs), _native.ptr(pos), _native.ptr(prec),
                                                  _native.ptr(label), key, nl, _native.ptr(off), _native.ptr(vals),
                                                  ctypes.c_void_p(out.data_ptr())), "mt_find_tiles_device")
        return out

    def find_markers_by_id(self, docs, ids, interner=None):
        """SharedString.getMarkerFromId(id) for each (doc, id): the marker row, removed or not,
        whose markerId property is the id (row -1: none in the tree; flags MT_MARK_DUP: several
        rows carry it, the first one answers).  An id the interner has never seen is in no
        document."""
        if interner is None:
            raise ValueError("find_markers_by_id: pass the interner the batches were encoded with")
        if docs is not None:
            docs = np.ascontiguousarray(docs, dtype=np.uint32).reshape(-1)
        n = len(docs) if docs is not None else self.n_docs
        ids = [ids] * n if isinstance(ids, str) else list(ids)
        if len(ids) != n:
            raise ValueError("find_markers_by_id: one id per query")
        from .wire import canonical_json
        none = 0xFFFFFFFF
        known = {} if interner.synthetic else interner.val_ids
        # (a falsy id is never mapped: MT/mergeTree.ts:281, :2109)
        val = np.ascontiguousarray([known.get(canonical_json(i), none) if i else none for i in ids], dtype=np.uint32)
        key = none if interner.synthetic else interner.key_ids.get(self.MARKER_ID_KEY, none)
        out = np.zeros(n, dtype=_native.SEG_HIT_DTYPE)
        self._check(self.lib.mt_find_markers_by_id(self.h, n, _native.ptr(docs), key, _native.ptr(val),
                                                   _native.ptr(out)), "mt_find_markers_by_id")
        return out

    def last_tiles(self):
        """(queries, rows examined, kernel ms) of the last bulk marker query."""
        out = np.zeros(2, dtype=np.int64)
        ms = ctypes.c_float()
        self._check(self.lib.mt_last_tiles(self.h, _native.ptr(out), ctypes.byref(ms)), "mt_last_tiles")
        return int(out[0]), int(out[1]), float(ms.value)

    # bulk ranged segment walk (mt_walk_segments): SharedSegmentSequence.walkSegments(handler,
    # start, end) for many (doc, start, end) queries in one counting pass and one gather
    def _walk_queries(self, docs, start, end, text, props):
        """(n, docs, start, end, what) as mt_walk_segments takes them; None entries of start are
        0, of end the document's length."""
        if isinstance(start, (list, tuple)):
            start = [0 if s is None else s for s in start]
        n, docs, start, end, _ = self._text_queries(docs, start, end, 0)
        what = (_native.MT_WALK_TEXT if text else 0) | (_native.MT_WALK_PROPS if props else 0)
        return n, docs, start, end, what

    @staticmethod
    def _view_cols(n, ref_seq, client):
        """ref_seq / client as mt_walk_segments_view takes them: None stays NULL, scalars broadcast."""
        return tuple(None if x is None else np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=np.int32), (n,)))
                     for x in (ref_seq, client))

    def walk_segments(self, docs=None, start=None, end=None, text=True, props=True, ref_seq=None, client=None):
        """(row_off, rows, text_off, text, word_off, records): query q's visited rows, in document
        order, are rows[row_off[q]:row_off[q + 1]] (WALK_ROW_DTYPE).  A row is visited when its
        observer length is > 0, its position is < end and its position + length is > start
        (nothing is clamped: start == end inside a segment visits it).  A text row's whole text
        is text[text_off[q] + row.text:][:row.length] (UTF-16 units), its property record
        [count, (key, value) x count] starts at records[word_off[q] + row.props]; either field
        is 0xFFFFFFFF when there is none or it was not asked for.  Queries as in get_texts.
        ref_seq / client (one value, or one per query): MergeTree.mapRange's view -- lengths,
        positions, start and end are then the (refSeq, client) view's (mt_walk_segments_view);
        client 0 is the replica's own view; rows of a query answered on the host carry
        MT_WALK_HOST in `flags`."""
        n, docs, start, end, what = self._walk_queries(docs, start, end, text, props)
        row_off, text_off, word_off = (np.zeros(n + 1, dtype=np.int64) for _ in range(3))
        fn, name, view = self.lib.mt_walk_segments, "mt_walk_segments", ()
        if ref_seq is not None or client is not None:
            fn, name = self.lib.mt_walk_segments_view, "mt_walk_segments_view"
            cols = self._view_cols(n, ref_seq, client)   # (kept alive for the calls below)
            view = tuple(_native.ptr(x) for x in cols)
        args = (self.h, n, _native.ptr(docs), _native.ptr(start), _native.ptr(end)) + view + (
            what, _native.ptr(row_off), _native.ptr(text_off), _native.ptr(word_off))
        self._check(fn(*args, None, 0, None, 0, None, 0), name)
        nr, nt, nw = int(row_off[n]), int(text_off[n]), int(word_off[n])
        rows = np.zeros(max(nr, 1), dtype=_native.WALK_ROW_DTYPE)
        units = np.zeros(max(nt, 1), dtype=np.uint16)
        recs = np.zeros(max(nw, 1), dtype=np.uint32)
        self._check(fn(*args, _native.ptr(rows), nr, _native.ptr(units), nt, _native.ptr(recs), nw), name)
        return row_off, rows[:nr], text_off, units[:nt], word_off, recs[:nw]

    def walk_segments_device(self, docs=None, start=None, end=None, text=True, props=True, out=None, ref_seq=None,
                             client=None):
        """walk_segments with the results left on the handle's device: (row_off, rows, text_off,
        text, word_off, records) torch tensors (int64 [n + 1] offsets; rows int32 [R, 12] holding
        the records' words, text int16, records int32).  out: (rows, text, records) tensors of
        those types on that device to fill (at least the results' sizes); the results are then
        their leading slices.  (torch is imported before the first handle is created, as for
        get_texts_device.)  ref_seq / client as in walk_segments."""
        import torch
        n, docs, start, end, what = self._walk_queries(docs, start, end, text, props)
        dev = torch.device("cuda", self.device)
        row_off, text_off, word_off = (torch.empty(n + 1, dtype=torch.int64, device=dev) for _ in range(3))
        fn, name, view = self.lib.mt_walk_segments_device, "mt_walk_segments_device", ()
        if ref_seq is not None or client is not None:
            fn, name = self.lib.mt_walk_segments_view_device, "mt_walk_segments_view_device"
            cols = self._view_cols(n, ref_seq, client)   # (kept alive for the calls below)
            view = tuple(_native.ptr(x) for x in cols)
        args = (self.h, n, _native.ptr(docs), _native.ptr(start), _native.ptr(end)) + view + (
            what, ctypes.c_void_p(row_off.data_ptr()), ctypes.c_void_p(text_off.data_ptr()),
            ctypes.c_void_p(word_off.data_ptr()))
        if out is None:
            self._check(fn(*args, None, 0, None, 0, None, 0), name)
            rows = torch.empty((max(int(row_off[n]), 1), 12), dtype=torch.int32, device=dev)
            units = torch.empty(max(int(text_off[n]), 1), dtype=torch.int16, device=dev)
            recs = torch.empty(max(int(word_off[n]), 1), dtype=torch.int32, device=dev)
        else:
            rows, units, recs = out
            for t, dt in ((rows, torch.int32), (units, torch.int16), (recs, torch.int32)):
                if t.dtype != dt or t.device != dev or not t.is_contiguous():
                    raise ValueError("walk_segments_device: out holds contiguous int32 / int16 / int32 tensors on "
                                     "the handle's device")
            if rows.dim() != 2 or rows.shape[1] != 12 or units.dim() != 1 or recs.dim() != 1:
                raise ValueError("walk_segments_device: out is (rows [R, 12], text [units], records [words])")
        self._check(fn(*args, ctypes.c_void_p(rows.data_ptr()), rows.shape[0], ctypes.c_void_p(units.data_ptr()),
                       units.numel(), ctypes.c_void_p(recs.data_ptr()), recs.numel()), name)
        return (row_off, rows[: int(row_off[n])], text_off, units[: int(text_off[n])], word_off,
                recs[: int(word_off[n])])

    def last_walk(self):
        """Device time (ms) of the last walk_segments call's counting pass and gather."""
        out = np.zeros(2, dtype=np.float32)
        self._check(self.lib.mt_last_walk_ms(self.h, _native.ptr(out)), "mt_last_walk_ms")
        return float(out[0]), float(out[1])

    def last_walk_view(self):
        """(queries, of them answered on the host, remote queries that started by a page skip,
        count ms, gather ms) of the last walk_segments / walk_segments_device call."""
        out = np.zeros(3, dtype=np.int64)
        ms = np.zeros(2, dtype=np.float32)
        self._check(self.lib.mt_last_walk_view(self.h, _native.ptr(out), _native.ptr(ms)), "mt_last_walk_view")
        return int(out[0]), int(out[1]), int(out[2]), float(ms[0]), float(ms[1])

    def get_texts_view(self, docs, start, end, ref_seq, client, placeholder=""):
        """MergeTreeTextHelper.getText(refSeq, clientId, placeholder, start, end) for each query,
        built on the host from one walk_segments call in the view, as gatherText clips
        (MT/textSegment.ts:241-263): a visited text row gives its whole text when start <= 0 and
        end >= its length, else substring(max(start, 0)) when end >= its length, else
        substring(start, end) with JavaScript's swap of the two when end < start; a marker gives
        the placeholder once per unit of its length ("" gives nothing; "*" is not offered)."""
        if placeholder == "*":
            raise ValueError('get_texts_view: the "*" placeholder is not offered')
        row_off, rows, text_off, units, _, _ = self.walk_segments(docs, start, end, props=False, ref_seq=ref_seq,
                                                                  client=client)
        raw = units.tobytes()
        out = []
        for q in range(len(row_off) - 1):
            t0, parts = int(text_off[q]), []
            for r in rows[int(row_off[q]):int(row_off[q + 1])]:
                ln, s, e = int(r["length"]), int(r["start"]), int(r["end"])
                if r["marker_ref_type"] >= 0:
                    parts.append(placeholder * ln)
                    continue
                lo = t0 + int(r["text"])
                text = raw[2 * lo: 2 * (lo + ln)].decode("utf-16-le", errors="surrogatepass")
                if s <= 0 and e >= ln:
                    parts.append(text)
                    continue
                s = max(s, 0)
                if e >= ln:
                    parts.append(text[s:])
                else:   # String.prototype.substring: both clamped into [0, length], swapped when start > end
                    a, b = min(max(s, 0), ln), min(max(e, 0), ln)
                    parts.append(text[min(a, b):max(a, b)])
            out.append("".join(parts))
        return out

    def get_prop_runs(self, doc):
        nr, nw = ctypes.c_uint32(), ctypes.c_uint32()
        self._check(self.lib.mt_get_prop_runs(self.h, doc, None, 0, ctypes.byref(nr), None, 0,
                                              ctypes.byref(nw)), "mt_get_prop_runs")
        runs = np.zeros((max(nr.value, 1), 3), dtype=np.uint32)
        recs = np.zeros(max(nw.value, 1), dtype=np.uint32)
        self._check(self.lib.mt_get_prop_runs(self.h, doc, _native.ptr(runs), nr.value, ctypes.byref(nr),
                                              _native.ptr(recs), nw.value, ctypes.byref(nw)),
                    "mt_get_prop_runs")
        out = []
        for s, l, r in runs[: nr.value].tolist():
            if r == 0xFFFFFFFF:
                out.append((s, l, None))
            else:
                n = int(recs[r])
                out.append((s, l, [(int(recs[r + 1 + 2 * j]), int(recs[r + 2 + 2 * j])) for j in range(n)]))
        return out

    # bulk / ranged property runs (mt_get_prop_runs_bulk): get_prop_runs clipped to [start, end)
    # for many documents in one counting pass and one gather on the device
    def get_prop_runs_raw(self, docs=None, start=None, end=None):
        """(run_off, word_off, runs[R, 3], records): query q's rows (position, length, record) are
        runs[run_off[q]:run_off[q + 1]]; a row's record [count, (key, value) x count] starts at
        records[word_off[q] + record] (record 0xFFFFFFFF: no properties).  Queries as in
        get_texts."""
        n, docs, start, end, _ = self._text_queries(docs, start, end, 0)
        run_off = np.zeros(n + 1, dtype=np.int64)
        word_off = np.zeros(n + 1, dtype=np.int64)
        args = (self.h, n, _native.ptr(docs), _native.ptr(start), _native.ptr(end), _native.ptr(run_off),
                _native.ptr(word_off))
        self._check(self.lib.mt_get_prop_runs_bulk(*args, None, 0, None, 0), "mt_get_prop_runs_bulk")
        nr, nw = int(run_off[n]), int(word_off[n])
        runs = np.zeros((max(nr, 1), 3), dtype=np.uint32)
        recs = np.zeros(max(nw, 1), dtype=np.uint32)
        self._check(self.lib.mt_get_prop_runs_bulk(*args, _native.ptr(runs), nr, _native.ptr(recs), nw),
                    "mt_get_prop_runs_bulk")
        return run_off, word_off, runs[:nr], recs[:nw]

    @staticmethod
    def _prop_run_lists(run_off, word_off, runs, recs):
        rows, words = runs.tolist(), recs.tolist()
        out = []
        for q in range(len(run_off) - 1):
            w0 = int(word_off[q])
            res = []
            for s, l, r in rows[int(run_off[q]): int(run_off[q + 1])]:
                if r == 0xFFFFFFFF:
                    res.append((s, l, None))
                else:
                    r += w0
                    res.append((s, l, [(words[r + 1 + 2 * j], words[r + 2 + 2 * j]) for j in range(words[r])]))
            out.append(res)
        return out

    def get_prop_runs_bulk(self, docs=None, start=None, end=None):
        """get_prop_runs-shaped lists (position, length, pairs | None), one per query
        (doc, start, end): every document when docs is None, whole documents when start / end
        are None (an end of -1 or None: the document's length).  start and end are clamped into
        [0, length]; positions stay document coordinates."""
        return self._prop_run_lists(*self.get_prop_runs_raw(docs, start, end))

    def get_properties_at_positions(self, docs, positions):
        """The property pairs (or None) at each (doc, position): one bulk call with ranges of
        width 1.  A position outside [0, length) answers None."""
        pos = np.asarray(positions, dtype=np.int64).reshape(-1)
        ok = (pos >= 0) & (pos < 0x7FFFFFFF)   # (position + 1 stays an int32)
        start = np.where(ok, pos, 0).astype(np.int32)
        end = np.where(ok, pos + 1, 0).astype(np.int32)
        docs = np.broadcast_to(np.asarray(docs, dtype=np.uint32), pos.shape)
        return [r[0][2] if r else None for r in self.get_prop_runs_bulk(docs, start, end)]

    def get_prop_runs_device(self, docs=None, start=None, end=None, out=None):
        """get_prop_runs_raw with the results left on the handle's device: (run_off, word_off,
        runs, records) torch tensors (int64 [n + 1] twice, int32 [R, 3] and int32 [W] holding the
        uint32 words).  out: (runs, records) int32 tensors on that device to fill (at least the
        results' sizes; runs of shape [rows, 3]); the results are then their leading slices.
        (torch is imported before the first handle is created, as for get_texts_device.)"""
        import torch
        n, docs, start, end, _ = self._text_queries(docs, start, end, 0)
        dev = torch.device("cuda", self.device)
        run_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        word_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        args = (self.h, n, _native.ptr(docs), _native.ptr(start), _native.ptr(end),
                ctypes.c_void_p(run_off.data_ptr()), ctypes.c_void_p(word_off.data_ptr()))
        if out is None:
            self._check(self.lib.mt_get_prop_runs_bulk_device(*args, None, 0, None, 0), "mt_get_prop_runs_bulk_device")
            runs = torch.empty((max(int(run_off[n]), 1), 3), dtype=torch.int32, device=dev)
            recs = torch.empty(max(int(word_off[n]), 1), dtype=torch.int32, device=dev)
        else:
            runs, recs = out
            for t in (runs, recs):
                if t.dtype != torch.int32 or t.device != dev or not t.is_contiguous():
                    raise ValueError("get_prop_runs_device: out holds contiguous int32 tensors on the handle's device")
            if runs.dim() != 2 or runs.shape[1] != 3 or recs.dim() != 1:
                raise ValueError("get_prop_runs_device: out is (runs [rows, 3], records [words])")
        self._check(self.lib.mt_get_prop_runs_bulk_device(*args, ctypes.c_void_p(runs.data_ptr()), runs.shape[0],
                                                          ctypes.c_void_p(recs.data_ptr()), recs.numel()),
                    "mt_get_prop_runs_bulk_device")
        return run_off, word_off, runs[: int(run_off[n])], recs[: int(word_off[n])]

    def last_props_ms(self):
        """Device time (ms) of the last bulk property-run call's counting pass and gather."""
        out = np.zeros(2, dtype=np.float32)
        self._check(self.lib.mt_last_props_ms(self.h, _native.ptr(out)), "mt_last_props_ms")
        return float(out[0]), float(out[1])

    def get_properties_at_position(self, doc, pos):
        return self.get_properties_at_positions([doc], [pos])[0]

    def debug_raw(self, doc):
        """Raw segment records (n x 8 u32: segA, segB) and the 32-word document header."""
        n = ctypes.c_uint32()
        hdr = np.zeros(32, dtype=np.int32)
        self._check(self.lib.mt_debug_raw(self.h, doc, None, 0, ctypes.byref(n), _native.ptr(hdr)), "mt_debug_raw")
        rows = np.zeros((max(n.value, 1), 8), dtype=np.uint32)
        self._check(self.lib.mt_debug_raw(self.h, doc, _native.ptr(rows), n.value, ctypes.byref(n), None),
                    "mt_debug_raw")
        return rows[:n.value], hdr

    def debug_props_sigs(self, doc):
        """The property-set signature each segment row carries (mt_debug_props_sigs)."""
        n = ctypes.c_uint32()
        self._check(self.lib.mt_debug_props_sigs(self.h, doc, None, 0, ctypes.byref(n)), "mt_debug_props_sigs")
        sigs = np.zeros(max(n.value, 1), dtype=np.uint32)
        self._check(self.lib.mt_debug_props_sigs(self.h, doc, _native.ptr(sigs), n.value, ctypes.byref(n)),
                    "mt_debug_props_sigs")
        return sigs[:n.value]

    def is_paged(self, doc):
        """True when the document lives in the paged layout (DESIGN.md 'Paged documents')."""
        return bool(self.debug_raw(doc)[1][24])

    def get_delta_log(self, doc):
        """The document's delta-log records since the last reset (oracle layout); raises
        DeltaLogOverflow when records were dropped (delta_log_capacity too small)."""
        n = ctypes.c_uint32()
        buf = np.zeros(1, dtype=np.int32)
        rc = self.lib.mt_get_delta_log(self.h, doc, None, 0, ctypes.byref(n))
        if rc not in (0, _native.MT_E_OVERFLOW):
            self._check(rc, "mt_get_delta_log")
        buf = np.zeros(max(n.value, 1), dtype=np.int32)
        rc = self.lib.mt_get_delta_log(self.h, doc, _native.ptr(buf), n.value, ctypes.byref(n))
        if rc == _native.MT_E_OVERFLOW:
            raise DeltaLogOverflow(self.lib.mt_last_error(self.h).decode(), buf[: n.value].tolist())
        self._check(rc, "mt_get_delta_log")
        return buf[: n.value].tolist()

    def delta_log_reset(self):
        """Empties every document's delta log (after its records were consumed)."""
        self._check(self.lib.mt_delta_log_reset(self.h), "mt_delta_log_reset")

    # bulk delta-log drain (mt_get_delta_logs): get_delta_log for many documents in one counting
    # pass and one gather on the device, optionally with one row per delta segment
    def _dlog_queries(self, docs, from_word):
        if docs is not None:
            docs = np.ascontiguousarray(docs, dtype=np.uint32).reshape(-1)
        n = len(docs) if docs is not None else self.n_docs
        if from_word is not None:
            from_word = np.ascontiguousarray(np.broadcast_to(np.asarray(from_word, dtype=np.int32), (n,)))
        return n, docs, from_word

    def get_delta_logs(self, docs=None, from_word=None, ranges=False):
        """(off, words, flags) -- with ranges, (off, words, row_off, rows, flags): query q's words
        are words[off[q]:off[q + 1]], the log of document docs[q] (every document when docs is
        None) from word from_word[q] (None: 0) on; rows[row_off[q]:row_off[q + 1]] are its delta
        segments (_native.DELTA_RANGE_DTYPE).  An overflowed document does not raise: flags[q]
        carries _native.MT_DLOG_OVERFLOWED (MT_DLOG_PAST: from_word beyond the log; MT_DLOG_BAD:
        from_word not a record boundary, no rows)."""
        n, docs, from_word = self._dlog_queries(docs, from_word)
        off = np.zeros(n + 1, dtype=np.int64)
        row_off = np.zeros(n + 1, dtype=np.int64) if ranges else None
        flags = np.zeros(max(n, 1), dtype=np.uint32)
        args = (self.h, n, _native.ptr(docs), _native.ptr(from_word), _native.ptr(off), _native.ptr(row_off),
                _native.ptr(flags))
        self._check(self.lib.mt_get_delta_logs(*args, None, 0, None, 0), "mt_get_delta_logs")
        nw, nr = int(off[n]), int(row_off[n]) if ranges else 0
        words = np.zeros(max(nw, 1), dtype=np.int32)
        rows = np.zeros(max(nr, 1), dtype=_native.DELTA_RANGE_DTYPE) if ranges else None
        self._check(self.lib.mt_get_delta_logs(*args, _native.ptr(words), nw, _native.ptr(rows), nr),
                    "mt_get_delta_logs")
        if ranges:
            return off, words[:nw], row_off, rows[:nr], flags[:n]
        return off, words[:nw], flags[:n]

    def get_delta_logs_device(self, docs=None, from_word=None, ranges=False):
        """get_delta_logs with the results left on the handle's device: torch tensors off (int64
        [n + 1]), words (int32), with ranges row_off (int64 [n + 1]) and rows (int32 [R, 8], the
        words of mt_delta_range), and flags (int32 [n] holding the uint32 flags).  (torch is
        imported before the first handle is created, as for get_texts_device.)"""
        import torch
        n, docs, from_word = self._dlog_queries(docs, from_word)
        dev = torch.device("cuda", self.device)
        off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        row_off = torch.empty(n + 1, dtype=torch.int64, device=dev) if ranges else None
        flags = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        args = (self.h, n, _native.ptr(docs), _native.ptr(from_word), ctypes.c_void_p(off.data_ptr()),
                ctypes.c_void_p(row_off.data_ptr()) if ranges else None, ctypes.c_void_p(flags.data_ptr()))
        self._check(self.lib.mt_get_delta_logs_device(*args, None, 0, None, 0), "mt_get_delta_logs_device")
        nw, nr = int(off[n]), int(row_off[n]) if ranges else 0
        words = torch.empty(max(nw, 1), dtype=torch.int32, device=dev)
        rows = torch.empty((max(nr, 1), _native.DELTA_RANGE_DTYPE.itemsize // 4), dtype=torch.int32, device=dev)
        self._check(self.lib.mt_get_delta_logs_device(*args, ctypes.c_void_p(words.data_ptr()), nw,
                                                      ctypes.c_void_p(rows.data_ptr()) if ranges else None, nr),
                    "mt_get_delta_logs_device")
        if ranges:
            return off, words[:nw], row_off, rows[:nr], flags[:n]
        return off, words[:nw], flags[:n]

    def delta_log_reset_docs(self, docs):
        """delta_log_reset for the listed documents only (the others keep their records)."""
        docs = np.ascontiguousarray(docs, dtype=np.uint32).reshape(-1)
        self._check(self.lib.mt_delta_log_reset_docs(self.h, len(docs), _native.ptr(docs)), "mt_delta_log_reset_docs")

    def last_dlog_ms(self):
        """Device time (ms) of the last get_delta_logs call's counting pass (with the walk of the
        records when rows were asked for) and gather."""
        out = np.zeros(2, dtype=np.float32)
        self._check(self.lib.mt_last_dlog_ms(self.h, _native.ptr(out)), "mt_last_dlog_ms")
        return float(out[0]), float(out[1])

    def maintenance_counts(self):
        """[n_docs, 3] SPLIT / APPEND / UNLINK mergeTreeMaintenanceCallback event counts
        (needs delta_log_capacity > 0)."""
        out = np.zeros((self.n_docs, 3), dtype=np.uint32)
        self._check(self.lib.mt_maintenance_counts(self.h, _native.ptr(out)), "mt_maintenance_counts")
        return out

    # -------------------------------------------------------------- live-client handles
    def regenerate_pending(self, doc, cap=1 << 16, text_cap=1 << 20, props_cap=1 << 20):
        """mt_regenerate_pending: the ops rebuilt from the oldest pending segment group
        (records, text, props), or None when nothing is pending."""
        out = np.zeros(cap, dtype=_native.REGEN_DTYPE)
        text = np.zeros(text_cap, dtype=np.uint16)
        props = np.zeros(props_cap, dtype=np.uint32)
        n = ctypes.c_int32(0)
        self._check(self.lib.mt_regenerate_pending(self.h, doc, _native.ptr(out), cap, ctypes.byref(n),
                                                   _native.ptr(text), text_cap, _native.ptr(props), props_cap),
                    "mt_regenerate_pending")
        if n.value < 0:
            return None
        return out[:n.value], text, props

    def pending_counts(self):
        """[n_docs, 2]: collabWindow.localSeq and the pending segment groups per document."""
        out = np.zeros((self.n_docs, 2), dtype=np.int32)
        self._check(self.lib.mt_pending_counts(self.h, _native.ptr(out)), "mt_pending_counts")
        return out

    def checksums(self):
        out = np.zeros(self.n_docs, dtype=CHECKSUM_DTYPE)
        self._check(self.lib.mt_checksums(self.h, _native.ptr(out)), "mt_checksums")
        return out

    def checksums_device(self, device_ptr):
        self._check(self.lib.mt_checksums_device(self.h, ctypes.c_void_p(device_ptr)), "mt_checksums_device")


class DeviceBatch:
    """A batch of encoded messages resident in HBM (mt_batch)."""

    def __init__(self, owner, a, handle=None):
        self.owner = owner
        lib = owner.lib
        if handle is None:
            ops = np.ascontiguousarray(a["ops"], dtype=OP_DTYPE)
            off = np.ascontiguousarray(a["doc_off"], dtype=np.int64)
            text = np.ascontiguousarray(a["text"], dtype=np.uint16)
            props = np.ascontiguousarray(a["props"], dtype=np.uint32)
            handle = lib.mt_batch_upload(owner.h, _native.ptr(off), _native.ptr(ops), len(ops),
                                         _native.ptr(text), len(text), _native.ptr(props), len(props))
            if not handle:
                raise RuntimeError(f"mt_batch_upload failed: {lib.mt_last_error(owner.h).decode()}")
        self.b = handle
        self.n_ops = int(lib.mt_batch_num_ops(self.b))

    def apply_async(self):
        self.owner._check(self.owner.lib.mt_batch_apply_async(self.owner.h, self.b), "mt_batch_apply_async")

    def sizes(self):
        """(op records, text units, property words) of the batch."""
        n, t, p = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        self.owner.lib.mt_batch_sizes(self.b, ctypes.byref(n), ctypes.byref(t), ctypes.byref(p))
        return int(n.value), int(t.value), int(p.value)

    def download(self):
        lib = self.owner.lib
        n, t, p = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        lib.mt_batch_sizes(self.b, ctypes.byref(n), ctypes.byref(t), ctypes.byref(p))
        off = np.zeros(self.owner.n_docs + 1, dtype=np.int64)
        ops = np.zeros(n.value, dtype=OP_DTYPE)
        text = np.zeros(max(t.value, 1), dtype=np.uint16)
        props = np.zeros(max(p.value, 1), dtype=np.uint32)
        rc = lib.mt_batch_download(self.b, _native.ptr(off), _native.ptr(ops), _native.ptr(text),
                                   _native.ptr(props))
        if rc:
            raise RuntimeError("mt_batch_download failed")
        return dict(doc_off=off, ops=ops, text=text, props=props)

    def free(self):
        if self.b:
            self.owner.lib.mt_batch_free(self.b)
            self.b = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceSnapshots:
    """Decoded summaries resident in HBM (mt_snapshots)."""

    def __init__(self, owner, handle):
        self.owner, self.s = owner, handle

    def load_async(self):
        self.owner._check(self.owner.lib.mt_snapshots_load_async(self.owner.h, self.s), "mt_snapshots_load_async")

    def free(self):
        if self.s:
            self.owner.lib.mt_snapshots_free(self.s)
            self.s = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
