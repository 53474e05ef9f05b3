"""Model-walk driver: drop-in for the reference's quant/gptq/src/quantizer.py `Quantizer`.

Same constructor, same walk (embed -> blocks in order -> lm_head), same hook protocol
(forward hooks feed inp[0] of every regex-matched Linear to its handle), same data.pth
schema (quantizer.py:268-275).  MI355X-first differences, none of which changes results:
  * the Linears of a block go through `block_schedule.BlockSchedule`: Linears fed by the SAME input tensor
    (q/k/v, gate/up) share one Hessian accumulation and one all-reduce instead of 3/2 identical ones, the
    Hessians of a block are accumulated by grouped SYRK launches, and the independent input groups quantize
    concurrently on their own HIP streams;
  * with world_size > 1 the Linears of a block are assigned to owner ranks (LPT on
    R*C*(C+128)) and quantize concurrently; the 5 result tensors are broadcast from the
    owner (the reference computes everything on rank 0, gptq.py:158);
  * every data.pth is written ONCE, by the rank its index maps to (the reference lets every rank write the same
    file), by a writer thread behind a copy stream, so that the device-to-host copies and the file writes of
    block i overlap with the forwards of block i+1; `quantize()` returns after the last file of every rank is
    closed (final barrier).
  * fused experts (transformers 5.x `MixtralExperts`: two 3-D parameters, nothing to hook) that the regex names as
    `...experts.<e>.w{1,2,3}` are presented as nn.Linear views for the duration of their block (moe_calibration.py); their
    trees are written under the checkpoint's names (`block_sparse_moe.experts.<e>.w{1,2,3}`).
`Quantizer.timing` holds the split of the last `quantize()` call (host seconds per phase and, with
GQ_TIMING=gpu, HIP-event seconds per phase on the main stream).
"""
import atexit
import os
import queue
import sys
import threading
import time
from typing import Any, Dict, Iterable, List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import dist_utils, moe_calibration
from . import ops as _ops
from .block_schedule import BlockSchedule
from .forward_fused import fused_forward, level_of, reset_verdicts
from .gptq import GPTQ
from .model_utils import ForwardInterrupt, InputCollector, LINEAR_LAYERS, _to, select_layers
from .quant_utils import GGML_QUANT_SIZES, GGMLQuantizationType, dequantize_linear_weight


def _same(a, b) -> bool:
    if torch.is_tensor(a) or torch.is_tensor(b):
        return torch.is_tensor(a) and torch.is_tensor(b) and a.shape == b.shape and a.dtype == b.dtype and \
            (a.data_ptr() == b.data_ptr() or bool(torch.equal(a, b)))
    if isinstance(a, (tuple, list)) and isinstance(b, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict) and isinstance(b, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    return a is b or a == b


def _batch_block_inputs(input_args, input_kwargs, batch: int):
    """Merge runs of up to `batch` consecutive captured block inputs into one call: the hidden states (first
    positional argument, or kwargs["hidden_states"]) are concatenated along dim 0; everything else must be IDENTICAL
    across the run (position ids / embeddings, masks, flags) and is taken from its first sample.  Samples that do
    not fit (another length, another mask) stay calls of their own."""
    def hidden(a, kw):
        return a[0] if len(a) > 0 else kw.get("hidden_states")

    def rest(a, kw):
        return (tuple(a[1:]), {k: v for k, v in kw.items() if k != "hidden_states" or len(a) > 0})

    out_a, out_kw, i, n = [], [], 0, len(input_args)
    while i < n:
        j = i + 1
        h0 = hidden(input_args[i], input_kwargs[i])
        while j < n and j - i < batch and torch.is_tensor(h0) and h0.dim() >= 2:
            hj = hidden(input_args[j], input_kwargs[j])
            if not (torch.is_tensor(hj) and hj.shape == h0.shape and hj.dtype == h0.dtype
                    and _same(rest(input_args[i], input_kwargs[i]), rest(input_args[j], input_kwargs[j]))):
                break
            j += 1
        if j - i == 1:
            out_a.append(input_args[i])
            out_kw.append(input_kwargs[i])
        else:
            cat = torch.cat([hidden(input_args[k], input_kwargs[k]) for k in range(i, j)], dim=0)
            if len(input_args[i]) > 0:
                out_a.append((cat,) + tuple(input_args[i][1:]))
                out_kw.append(input_kwargs[i])
            else:
                out_a.append(input_args[i])
                out_kw.append(dict(input_kwargs[i], hidden_states=cat))
        i = j
    return out_a, out_kw


def _own_storage(t):
    """torch.save writes a tensor's WHOLE storage: a view into a larger buffer (a staging slot, the gathered block
    buffer of the N > 1 exchange) is copied out first."""
    return t if t.untyped_storage().nbytes() == t.numel() * t.element_size() else t.clone()


RAW_BYTES = -1  # the q_type of a saver item that is ONE uint8 tensor, written as it is to the absolute path `name`


def _write_data_pth(save_dir, name, q_type, qweight, d=None, s=None, dmin=None, m=None):
    if q_type == RAW_BYTES:  # a level of the level database: raw GGUF block bytes, no pickle (level_db.LevelDbWriter.register)
        qweight.contiguous().numpy().tofile(name)
        return
    os.makedirs(os.path.join(save_dir, name), exist_ok=True)
    qweight, d, s, dmin, m = (_own_storage(t) for t in (qweight, d, s, dmin, m))
    torch.save({"q_type": int(q_type), "qweight": qweight, "super_group_scale": d, "super_group_zero": dmin,
                "group_scale_quant": s, "group_zero_quant": m}, os.path.join(save_dir, name, "data.pth"))


def _layout_of(tensors, off):
    """(offset, bytes, dtype, shape) of each tensor packed from `off` on, 256-byte aligned; and the end offset."""
    layout = []
    for t in tensors:
        n = t.numel() * t.element_size()
        layout.append((off, n, t.dtype, tuple(t.shape)))
        off += (n + 255) & ~255
    return layout, off


def _slot_views(slot, layout):
    return [slot[off:off + n].view(dt).view(shape) for off, n, dt, shape in layout]


def _writer_process(save_dir, slots, inbox, freeq, outbox):
    """Body of the writer PROCESS.  `slots` are the parent's pinned staging buffers (shared memory): a message names
    a slot and the layout of a module's five tensors inside it; they are copied out, the slot goes back to the parent,
    then torch.save runs here -- with this process's interpreter lock, not the parent's."""
    failed = None
    busy = 0.0
    try:
        torch.set_num_threads(1)
        while True:
            item = inbox.get()
            if item is None:
                break
            t0 = time.perf_counter()
            try:
                if item[0] == "slots":  # one staging slot holding the tensors of one or more modules
                    _, sid, modules = item
                    name = modules[0][0]
                    try:
                        hosts = [[v.clone() for v in _slot_views(slots[sid], layout)] for _, _, layout in modules] \
                            if failed is None else []
                    finally:
                        freeq.put(sid)  # ALWAYS handed back: the parent must never wait on a writer that failed
                    for (name, q_type, _), host in zip(modules, hosts):
                        if failed is None:
                            _write_data_pth(save_dir, name, q_type, *host)
                    hosts = None
                    host = None
                else:  # a module larger than a slot: its host tensors came through the queue
                    _, name, q_type, host = item
                    if failed is None:
                        _write_data_pth(save_dir, name, q_type, *host)
            except BaseException as e:  # disk full, unwritable save_dir, ...: reported at once, later items are dropped
                if failed is None:
                    failed = f"{name}: {e!r}"
                    outbox.put(("error", failed))
            del item
            host = None
            busy += time.perf_counter() - t0
        outbox.put(("ok", busy) if failed is None else ("error", failed))
    except BaseException as e:  # reported to the parent
        outbox.put(("error", repr(e)))


class _Saver:
    """data.pth writer (quantizer.py:267-275) off the critical path.  The calling thread copies a block's result
    tensors into a pinned staging slot with copy kernels on its own stream (put_many: why not a side thread's stream);
    the slots live in shared memory; a copier thread waits for the copies on the host and a separate PROCESS copies the
    slot out and runs torch.save.  Why a process: torch.save holds the interpreter lock for much of its 0.7 s per GB and
    Llama-3-8B leaves 8.7 GB of data.pth behind -- written from a thread of this process, the launches of the next
    block's forwards stall; why pinned slots: fresh pageable host tensors cost 6-9 s in page faults.
    `_Saver.USE_PROCESS = False` keeps everything in-process; `sync=True` (CPU tensors) writes in line like the reference."""

    USE_PROCESS, KERNEL_COPY, INLINE = True, True, True
    _teardowns: List[threading.Thread] = []  # deferred close() tails still running (see close / _join_teardowns)

    @staticmethod
    def _join_teardowns(timeout: float = 90.0) -> None:
        while _Saver._teardowns:
            _Saver._teardowns.pop().join(timeout=timeout)

    def __init__(self, save_dir: str, sync: bool):
        self.save_dir, self.sync = save_dir, sync
        self.q: "queue.Queue" = queue.Queue()
        self.err: Optional[BaseException] = None
        self.busy_s = 0.0
        self.thread = None
        self.proc = self.inbox = self.outbox = self.freeq = None
        self.slots: List[torch.Tensor] = []
        self._writer_dead = False
        self._final = None
        # class-level switches (profiles/ probes flip them; the measured alternatives are in DESIGN.md 6b): torch.save in a
        # writer PROCESS (False: in this process's copier thread), copy kernels through the slot's device mapping (False:
        # hipMemcpyAsync), staged by the caller's thread on its own stream (False: by the copier thread on a stream of its own
        # -- which puts the run into the slow mode of DESIGN.md 6b)
        self.use_process, self._kernel_copy, self._inline = _Saver.USE_PROCESS, _Saver.KERNEL_COPY, _Saver.INLINE
        self.n_slots = max(2, int(os.environ.get("GQ_SAVE_SLOTS", 3)))
        self._ready = threading.Event()
        self._poll_lock = threading.Lock()
        self._pinned_ids = set()
        self.slot_bytes = int(os.environ.get("GQ_SAVE_SLOT_MB", 704)) << 20  # embed_tokens of Llama-3 in Q4_K: 657 MB

    def _start_process(self):
        import torch.multiprocessing as tmp
        ctx = tmp.get_context("spawn")
        _Saver._join_teardowns()  # a previous saver's slots (2.1 GB of /dev/shm) are gone before this one asks for room
        # the slots are files in /dev/shm: ftruncate succeeds on a small tmpfs (Docker's default is 64 MB) and the
        # first write into the slot then kills the process with SIGBUS -- ask before allocating
        need = self.n_slots * self.slot_bytes + (64 << 20)
        try:
            st = os.statvfs("/dev/shm")
            free = st.f_bavail * st.f_frsize
        except OSError:
            free = 0
        if free < need:
            raise OSError(f"/dev/shm has {free >> 20} MiB free, the writer process needs {need >> 20} MiB "
                          f"(GQ_SAVE_SLOT_MB={self.slot_bytes >> 20})")
        # slots: shared-memory storages created as such (share_memory_() on an ordinary tensor would copy 704 MB each);
        # nothing touches their pages until they are pinned
        def new_slot():
            try:
                return torch.empty(0, dtype=torch.uint8).set_(torch.UntypedStorage._new_shared(self.slot_bytes))
            except Exception:
                return torch.empty(self.slot_bytes, dtype=torch.uint8).share_memory_()
        self.slots = [new_slot() for _ in range(self.n_slots)]
        self._registered = []
        self._pinned_ids = set()
        self.inbox, self.outbox, self.freeq = ctx.Queue(), ctx.Queue(), ctx.Queue()
        self.proc = ctx.Process(target=_writer_process, args=(self.save_dir, self.slots, self.inbox, self.freeq, self.outbox),
                                daemon=True)
        self.proc.start()  # the child imports torch while the slots are pinned here
        for sid, t in enumerate(self.slots):  # pin the shared pages: the copy kernels write through their device mapping
            try:
                if int(torch.cuda.cudart().cudaHostRegister(t.data_ptr(), t.numel(), 0)) == 0:
                    self._registered.append(t)
                    self._pinned_ids.add(sid)
                else:
                    self._kernel_copy = False  # an unpinned slot has no device mapping: hipMemcpyAsync stages it
            except Exception:
                self._kernel_copy = False
            self.freeq.put(sid)
            self._ready.set()  # the first slot is enough to start with (embed_tokens); the others follow

    def _loop(self):
        stream = None
        while True:
            item = self.q.get()
            if item is None:
                return
            try:
                t0 = time.perf_counter()
                if item[0] == "staged":
                    # the main thread's copy kernels filled slot `sid` behind `ev` (put_many): wait for them on the host
                    # and hand the slot to the writer
                    _, sid, modules, ev = item
                    sent = False
                    try:
                        ev.synchronize()
                        self.inbox.put(("slots", sid, modules))
                        sent = True
                    finally:
                        if not sent:
                            self.freeq.put(sid)
                    self.busy_s += time.perf_counter() - t0
                    continue
                if item[0] == "host":
                    _, name, q_type, host = item
                    if self.proc is not None and not self._writer_dead:
                        self.inbox.put(("host", name, int(q_type), host))
                    else:
                        _write_data_pth(self.save_dir, name, q_type, *host)
                    self.busy_s += time.perf_counter() - t0
                    continue
                _, name, q_type, tensors, ev, dev = item
                if stream is None:
                    stream = torch.cuda.Stream(dev)
                layout, off = _layout_of(tensors, 0)
                # host-side wait (no interpreter lock held): nothing is parked on a hardware queue before the results exist
                ev.synchronize()
                with torch.cuda.stream(stream):
                    sid = self._get_slot() if (self.proc is not None and off <= self.slot_bytes) else None
                    if sid is not None:
                        sent = False
                        try:
                            for v, t in zip(_slot_views(self.slots[sid], layout), tensors):
                                if self._kernel_copy:
                                    _ops.stage_to_host(v, t.contiguous(), stream)
                                else:
                                    v.copy_(t.contiguous(), non_blocking=True)
                            stream.synchronize()
                            self.inbox.put(("slots", sid, [(name, int(q_type), layout)]))
                            sent = True
                        finally:
                            if not sent:  # an exception between taking the slot and handing it over: no leak
                                self.freeq.put(sid)
                    else:
                        host = [t.cpu() for t in tensors]
                        if self.proc is not None and not self._writer_dead:
                            self.inbox.put(("host", name, int(q_type), host))
                        else:
                            _write_data_pth(self.save_dir, name, q_type, *host)
                del tensors, item
                self.busy_s += time.perf_counter() - t0
            except BaseException as e:  # surfaced by close()
                self.err = self.err or e

    def _poll_writer(self) -> None:
        """Non-blocking look at the writer: an error message or a dead process switches to in-thread writing (the
        failed file is reported by close(); nothing ever waits on a writer that cannot answer)."""
        if self.proc is None or self._writer_dead:
            return
        with self._poll_lock:  # the main thread (put_many) and the copier thread both look
            try:
                while True:
                    status, info = self.outbox.get_nowait()
                    if status == "error":
                        self._writer_failed(info)
                    else:
                        self._final = (status, info)
            except queue.Empty:
                pass
            if self._final is None and not self._writer_dead and not self.proc.is_alive():
                self._writer_failed(f"writer process exited with code {self.proc.exitcode}")

    def _writer_failed(self, info) -> None:
        self._writer_dead = True
        self.err = self.err or RuntimeError(f"data.pth writer process failed: {info}")

    def _get_slot(self):
        """A free staging slot, or None when the writer process is gone (the caller then writes in this thread)."""
        while True:
            self._poll_writer()
            if self._writer_dead:
                return None
            try:
                return self.freeq.get(timeout=1.0)
            except queue.Empty:
                continue

    def warm_up(self, device) -> None:
        """Start the writer process and pin its slots now (0.3 s), in the background of the capture forward."""
        if self.sync or self.thread is not None or torch.device(device).type != "cuda":
            return
        def boot():
            try:
                if self.use_process:
                    self._start_process()
            except BaseException as e:  # no writer process (small /dev/shm, spawn failure): this thread writes, as
                # _Saver.USE_PROCESS = False does -- a start-up problem of an optimisation is logged, not raised after hours
                dist_utils.print_on_main(f"[gq] data.pth writer process not started ({e}); writing from a thread")
                self.proc = None
                self.slots = []
            self._ready.set()
            self._loop()

        self.thread = threading.Thread(target=boot, name="gq-data-pth-copier", daemon=True)
        self.thread.start()

    def put(self, name, q_type, tensors):
        self.put_many([(name, q_type, tensors)])

    def put_many(self, items):
        """Queue the tensors of some modules (one transformer block's Linears, or embed / lm_head alone) for writing.
        Default path: THIS thread launches copy kernels (gq_stage_to_host) on its current stream, right behind the
        kernels that produce the tensors, into one pinned staging slot for the whole group; the copier thread only waits
        for them (on the host) and passes the slot to the writer process.  Measured on Llama-3-8B: a second thread
        launching ANYTHING on a stream of its own while this thread issues the forwards -- one 16-element fill per
        module is enough -- costs 2-3 s of a 12 s run (forward #1 5.8 -> 7.5 s, the chains 1.1 -> 1.6 s); GPU-side the
        copies are 5 ms per block either way.  In that slow mode the large kernels run as fast as ever (SYRK 1.77 vs 1.68 s
        per run) while the launches that hang on cross-stream events do not: the single-workgroup Cholesky leaves take
        574 vs 305 ms, the column-loop kernels 793 vs 590 ms (bench.py, GQ_BENCH_WM_PROF) -- dependent dispatch got slower,
        not the kernels; the cause inside the runtime is not identified (hardware-queue count, copy engine, PCIe and the
        allocator are ruled out: DESIGN.md 6b).  (_Saver.INLINE = False: the copier thread copies on its own stream.)"""
        if not items:
            return
        if self.sync or not items[0][2][0].is_cuda:
            for name, q_type, tensors in items:
                t0 = time.perf_counter()
                _write_data_pth(self.save_dir, name, q_type, *[t.cpu() for t in tensors])
                self.busy_s += time.perf_counter() - t0
            return
        dev = items[0][2][0].device
        if self.thread is None:
            self.warm_up(dev)
        cur = torch.cuda.current_stream(dev)
        self._ready.wait()  # the writer process is up (or known to be absent)
        inline = (self._inline and self.proc is not None and self._kernel_copy and not self._writer_dead)
        group, size = [], 0

        def flush():
            nonlocal group, size
            if not group:
                return
            # May wait for the writer to hand a slot back (that needs only work which is already queued: the copy kernels,
            # the copier's host-side wait, the writer's clone).  Waiting is the lesser evil: sending the group down the
            # copier thread's own-stream path instead was tried -- one early miss and the rest of the run is in the slow
            # mode (13.4 vs 12.1 s).  Three slots: a Llama block needs one per 350 ms, the writer frees one in 130 ms.
            sid = self._get_slot()
            if sid is None:
                for name, q_type, tensors in group:
                    self._put_one(name, q_type, tensors, cur, dev)
            else:
                sent = False
                try:
                    modules, off = [], 0
                    for name, q_type, tensors in group:
                        layout, off = _layout_of(tensors, off)
                        modules.append((name, int(q_type), layout))
                        for v, t in zip(_slot_views(self.slots[sid], layout), tensors):
                            if sid in self._pinned_ids:
                                _ops.stage_to_host(v, t.contiguous(), cur)
                            else:  # a slot that could not be pinned has no device mapping
                                v.copy_(t.contiguous(), non_blocking=True)
                    ev = torch.cuda.Event()
                    ev.record(cur)
                    self.q.put(("staged", sid, modules, ev))
                    sent = True
                finally:
                    if not sent:
                        self.freeq.put(sid)
            group, size = [], 0

        for name, q_type, tensors in items:
            n = _layout_of(tensors, 0)[1]
            if inline and n > self.slot_bytes:
                # larger than a slot (a 70B model's embed_tokens): copied out by THIS thread, synchronously -- twice per
                # model -- rather than by the copier on a stream of its own
                flush()
                self.q.put(("host", name, q_type, [t.cpu() for t in tensors]))
                continue
            if not inline:
                flush()
                self._put_one(name, q_type, tensors, cur, dev)
                continue
            if size + n > self.slot_bytes:
                flush()
            group.append((name, q_type, tensors))
            size += n
        flush()

    def _put_one(self, name, q_type, tensors, cur, dev):
        ev = torch.cuda.Event()
        ev.record(cur)
        self.q.put(("copy", name, q_type, tensors, ev, dev))

    def close(self):
        t0 = time.perf_counter()
        self.close_split = {}
        if self.thread is not None:
            self.q.put(None)
            while self.thread.is_alive():  # the copier never blocks for good (_get_slot polls the writer), but look anyway
                self.thread.join(timeout=5.0)
                self._poll_writer()
            self.thread = None
        self.close_split["copier_drained"] = round(time.perf_counter() - t0, 4)
        if self.proc is not None:
            self._poll_writer()
            status, info = "error", "no answer"
            try:
                self.inbox.put(None)
                deadline = time.time() + 600
                while self._final is None and time.time() < deadline:
                    try:
                        st, inf = self.outbox.get(timeout=0.05)
                        if st == "error" and not self._writer_dead:
                            self._writer_failed(inf)
                        self._final = (st, inf)
                    except queue.Empty:
                        if not self.proc.is_alive():
                            break
                if self._final is not None:
                    status, info = self._final
                elif not self.proc.is_alive():
                    info = f"writer process exited with code {self.proc.exitcode}"
            except Exception as e:
                info = f"writer process did not answer: {e!r}"
            self.close_split["writer_answered"] = round(time.perf_counter() - t0, 4)
            # every file is on disk once the writer has answered.  What is left -- the child's interpreter exit (it imported
            # torch: 0.2-0.4 s) and un-pinning three 704 MB slots -- needs nobody's attention: a daemon thread does it, the
            # slots stay referenced by it until then
            proc, registered, slots = self.proc, list(getattr(self, "_registered", [])), self.slots

            def _teardown():
                try:
                    proc.join(timeout=60)
                finally:
                    for t in registered:
                        try:
                            torch.cuda.cudart().cudaHostUnregister(t.data_ptr())
                        except Exception:
                            pass
                    slots.clear()
            if status == "ok" and not self._writer_dead:
                # joined by the next _Saver before it sizes /dev/shm, and at interpreter exit BEFORE the HIP runtime is
                # finalised (atexit hooks run ahead of module teardown): the thread never calls into a dying runtime
                th = threading.Thread(target=_teardown, daemon=True, name="gq-saver-teardown")
                _Saver._teardowns.append(th)
                th.start()
            else:
                _teardown()
            self._registered = []
            self.proc = self.inbox = self.outbox = self.freeq = None
            self.slots = []
            self.close_split["returned"] = round(time.perf_counter() - t0, 4)
            if status == "ok" and not self._writer_dead:
                self.writer_busy_s = float(info)
            else:
                self.err = self.err or RuntimeError(f"data.pth writer process failed: {info}")
        if self.err is not None:
            raise self.err


atexit.register(_Saver._join_teardowns, 30.0)


class _Phases:
    """Where the time of quantize() goes: host seconds per phase, plus GPU seconds per phase from HIP events on
    the main stream when GQ_TIMING=gpu (the events are read once, at the end)."""

    def __init__(self, device):
        self.host: Dict[str, float] = {}
        self.gpu_events: List[Any] = []
        self.use_gpu = os.environ.get("GQ_TIMING") == "gpu" and torch.device(device).type == "cuda"
        self.device = device
        self._t = time.perf_counter()
        self._e = self._event()

    def _event(self):
        if not self.use_gpu:
            return None
        e = torch.cuda.Event(enable_timing=True)
        e.record(torch.cuda.current_stream(self.device))
        return e

    def mark(self, phase: str):
        now = time.perf_counter()
        self.host[phase] = self.host.get(phase, 0.0) + now - self._t
        self._t = now
        if self.use_gpu:
            e = self._event()
            self.gpu_events.append((phase, self._e, e))
            self._e = e

    def result(self) -> Dict[str, Any]:
        out = {"host_s": {k: round(v, 4) for k, v in self.host.items()}}
        if self.use_gpu:
            torch.cuda.synchronize(self.device)
            g: Dict[str, float] = {}
            for phase, a, b in self.gpu_events:
                g[phase] = g.get(phase, 0.0) + a.elapsed_time(b) * 1e-3
            out["gpu_s"] = {k: round(v, 4) for k, v in g.items()}
        return out


def _first(x):
    return x[0] if isinstance(x, (tuple, list)) else x


def level_tree_name(level, module: str) -> str:
    """Where a module's data.pth of a level build lies under save_dir: <LEVEL>/<module> (the level's type name, e.g.
    Q4_K/model.layers.0.mlp.up_proj) -- <save_dir>/<LEVEL> is an ordinary tree, a valid --dir_model_quant of the packer."""
    return f"{GGMLQuantizationType(level).name}/{module}"


def check_levels(levels, propagate):
    """-> (levels, propagate) as GGMLQuantizationType (propagate None stays None); ValueError for an empty or repeated
    list or a propagate level that is not built."""
    levels = [GGMLQuantizationType(t) for t in levels]
    if not levels or len(set(levels)) != len(levels):
        raise ValueError("levels must be a non-empty list of distinct K-quant types")
    if propagate is not None:
        propagate = GGMLQuantizationType(propagate)
        if propagate not in levels:
            raise ValueError(f"propagate level {propagate.name} is not one of the levels {[t.name for t in levels]}")
    return levels, propagate


IQ4_LEVEL_TYPES = {"IQ4_XS": 23, "IQ4_NL": 20}  # the ggml type ids (include/gptq_gguf_iq4.h)


IQ4_LEVEL_METHODS = ("rtn", "gptq")


def check_iq4_levels(iq4, importance: str = "hessian", method: str = "rtn") -> Tuple[int, ...]:
    """-> the ggml type ids of `iq4` (names out of IQ4_XS / IQ4_NL, or their ids), in its order; ValueError for anything else,
    for an unknown importance or method, and for the method "gptq" without a type."""
    ids = []
    for t in iq4 or ():
        t = IQ4_LEVEL_TYPES.get(str(t).upper(), t)
        if t not in IQ4_LEVEL_TYPES.values() or t in ids:
            raise ValueError(f"level_db_iq4: {list(iq4)} (distinct types out of {list(IQ4_LEVEL_TYPES)})")
        ids.append(int(t))
    if importance not in ("hessian", "none"):
        raise ValueError(f"level_db_iq4_importance: {importance!r} (hessian or none)")
    if method not in IQ4_LEVEL_METHODS:
        raise ValueError(f"level_db_iq4_method: {method!r} (rtn or gptq)")
    if method != "rtn" and not ids:
        raise ValueError(f"level_db_iq4_method: {method!r} needs level_db_iq4 (there is no IQ4 level to build)")
    return tuple(ids)


class _LevelDbSink:
    """The level-database side of a level build (quant.py --level_db): packs every walk's bands into GGUF block bytes with
    ONE gq_pack_bands launch on the walk's stream -- q / k rows gathered into GGUF's rotary order on the way -- and books the
    files with level_db.LevelDbWriter; the bytes travel through the _Saver like a tree's tensors (RAW_BYTES items).  The
    key/value data and the tensors GPTQ does not quantize come from the model directory, by the converter's own rules
    (pack_gptq_into_gguf.add_model_metadata / plain_tensor with --outtype f16): the database is what converting every
    level's tree and splitting the files with --exact leaves.  Dense Llama family, dense Qwen3 (no q / k row gather) and Mixtral;
    the HF side is not written.
    `q8_0`: every tensor whose K-quant levels were packed also gets the 8.5-bit level 8.5-Q8_0.pth -- round-to-nearest of
    the checkpoint's unmodified weights (gq_quantize_q8_0, q / k rows gathered on the way), what `llama-quantize Q8_0` and
    the splitter would leave; GPTQ has no part in it.
    `iq4`: type names out of ("IQ4_XS", "IQ4_NL") -- every such tensor also gets the levels 4.25-IQ4_XS.pth / 4.56-IQ4_NL.pth,
    encoded from the block's unmodified weight by gq_quantize_iq4 (include/gptq_gguf_iq4_encode.h; q / k rows gathered on the
    way) ahead of its walk (`before_levels`, BlockSchedule.quantize_levels' `before`), registered BEFORE its K-quant levels so
    that the tensor's gguf_layer_database.json record stays its last K-quant level.  `iq4_importance` "hessian": a column's
    importance is the diagonal of the Linear's accumulated calibration Hessian, what llama.cpp calls the importance matrix;
    "none", and the tensors that have no Hessian (embed / lm_head): unweighted.  A tensor whose rows are no multiple of 256
    gets no IQ4_XS level.
    `iq4_method` "rtn" (the default): as above, no GPTQ error feedback.  "gptq": the IQ4 levels of a Linear come out of GPTQ's
    column walk on the IQ4 grid (gq_gptq_quantize_iq4, include/gptq_gguf_iq4_gptq.h) with the Linear's own
    factorisation: `before_levels` only keeps diag(H), `after_levels` (BlockSchedule.quantize_levels' `extra`, which runs ahead
    of `pack`, so the files are still registered before the K-quant levels) walks a fresh working copy once per type and packs
    it with gq_pack_iq4.  embed / lm_head have no Hessian and stay round-to-nearest, unweighted, under either method."""

    def __init__(self, db: str, dir_model: str, vocab: bool = True, q8_0: bool = False, iq4=(), iq4_importance: str = "hessian",
                 iq4_method: str = "rtn"):
        import json
        from pathlib import Path
        from . import level_db
        from .pack_gptq_into_gguf import SKIPPED_HF_TENSORS, gguf_arch, iter_hf_entries, map_tensor_name, rope_setup
        if not dir_model or not os.path.isdir(dir_model) or not os.path.isfile(os.path.join(dir_model, "config.json")):
            raise ValueError(f"level_db needs the model as a local directory with config.json and *.safetensors (got "
                             f"{dir_model!r}): the key/value data and the plain tensors are read from it")
        self.dir_model, self.vocab, self.q8_0 = Path(dir_model), vocab, bool(q8_0)
        self.iq4 = check_iq4_levels(iq4, iq4_importance, iq4_method)
        self.iq4_importance, self.iq4_method = iq4_importance, iq4_method
        self._iq4_imp: Dict[str, Optional[torch.Tensor]] = {}  # "gptq": diag(H) of a Linear between its two hooks
        self.hp = json.load(open(self.dir_model / "config.json"))
        arch = self.hp.get("architectures", ["LlamaForCausalLM"])[0]
        self.n_experts = int(self.hp.get("num_local_experts") or 0)
        dense = ("LlamaForCausalLM", "LLaMAForCausalLM", "MistralForCausalLM", "Qwen3ForCausalLM")
        if not ((arch in dense and not self.n_experts) or (arch == "MixtralForCausalLM" and self.n_experts)):
            raise NotImplementedError(f"level_db: {arch} (the dense Llama family, dense Qwen3, and MixtralForCausalLM with "
                                      "num_local_experts; Qwen3MoeForCausalLM and Qwen2ForCausalLM's biases are out of scope)")
        self.gguf_arch = gguf_arch(self.hp)  # "llama": q / k rows are stored in GGUF's rotary order; "qwen3": in place
        self.n_head = self.hp["num_attention_heads"]
        self.n_kv = self.hp.get("num_key_value_heads", self.n_head)
        _, self.rope_type = rope_setup(self.hp)
        self.tensor_of: Dict[str, str] = {}  # HF module name -> GGUF tensor name, for what the checkpoint holds
        # checkpoint name of an expert matrix (model.layers.N.block_sparse_moe.experts.<e>.w1) -> (unit tensor
        # blk.N.ffn_gate_exps.weight, slot e): the packer stacks the E matrices of a block and role into that one tensor
        self.expert_of: Dict[str, Tuple[str, int]] = {}
        order = ["rope_freqs.weight"] if self.rope_type == "llama3" else []
        self.total_params = self.expert_params = 0
        seen: Dict[str, int] = {}
        for name, shape, _ in iter_hf_entries(self.dir_model):
            if name.endswith(SKIPPED_HF_TENSORS):
                continue
            numel = int(np.prod(shape)) if len(shape) else 1
            self.total_params += numel
            if ".block_sparse_moe.experts." in name:  # (the converter's own rule and name arithmetic)
                parts = name.split(".")
                bid, xid, wid = int(parts[2]), int(parts[5]), parts[6]
                unit = map_tensor_name(f"layers.{bid}.feed_forward.experts.{wid}.weight")
                if len(shape) != 2 or shape[0] % 64:
                    raise NotImplementedError(f"level_db: {name} has shape {tuple(shape)}; an expert matrix whose rows are no "
                                              f"multiple of 64 cannot be packed into a slot of {unit}")
                self.expert_params += numel
                self.expert_of[name.removesuffix(".weight")] = (unit, xid)
                seen[unit] = seen.get(unit, 0) + 1
                if seen[unit] == self.n_experts:  # the converter adds the merged tensor with its last expert
                    order.append(unit)
                continue
            self.tensor_of[name.removesuffix(".weight")] = map_tensor_name(name)
            order.append(map_tensor_name(name))
        short = sorted(u for u, n in seen.items() if n != self.n_experts)
        if short:
            raise ValueError(f"level_db: {short[0]} has {seen[short[0]]} expert matrices in the checkpoint, config.json says "
                             f"{self.n_experts}")
        # (unit tensor, ggml type) -> [buffer [E, R, C / 256 * type_size], slots filled, path]; allocated on the first slice
        self.units: Dict[Tuple[str, int], list] = {}
        self.writer = level_db.LevelDbWriter(db)
        self.writer.set_order(order)
        self.packed = set()   # HF module names whose levels are in the database
        self.items: List[tuple] = []  # saver items of the walks packed since the last take()

    def _row_src(self, tensor: str, rows: int, device):
        from .gguf_loader import rotary_row_dst
        if self.gguf_arch != "llama":
            return None
        return rotary_row_dst(tensor, rows, self.n_head, self.n_kv, device)

    def pack_walk(self, stacked, bands, members):
        """One walk -> one launch (BlockSchedule.quantize_levels' `pack`; also the one-band calls of embed / lm_head and of
        the level-after-level walks).  members[k]: (HF module name, q_type) of band k, or None (stale: packed, not kept).
        Rows that are no multiple of 64 cannot lie in a band table: such a one-band walk takes gq_pack, its rows gathered
        first."""
        q = stacked[0]
        dev, C = q.device, q.shape[1]
        self.device = dev  # (finish() encodes the Q8_0 level where the walks ran)
        tensors = [None if mem is None else self.tensor_of.get(mem[0]) for mem in members]
        slots = [None if mem is None else self._slot_of(mem[0]) for mem in members]
        if any(sl is not None for sl in slots):
            return self._pack_expert_walk(stacked, bands, members, tensors, slots)
        if all(t is None for t in tensors):
            return []
        r0, srcs = 0, []
        for (r1, _), t in zip(bands, tensors):
            srcs.append(self._row_src(t, r1 - r0, dev) if t is not None else None)
            r0 = r1
        if len(bands) == 1 and bands[0][0] % 64:
            five = stacked if srcs[0] is None else [x.index_select(0, srcs[0].long()) for x in stacked]
            outs = [_ops.pack(bands[0][1], *five)]
        else:
            outs = _ops.pack_bands(stacked, bands, None, srcs)
        r0 = 0
        for (r1, t), mem, tensor, out in zip(bands, members, tensors, outs):
            if tensor is not None:
                path = self.writer.register(tensor, (r1 - r0, C), int(t))
                self.items.append((path, RAW_BYTES, (out.view(-1),)))
                self.packed.add(mem[0])
            r0 = r1
        return outs

    # ---- stacked expert units ----
    def _slot_of(self, name: str) -> Optional[Tuple[str, int]]:
        """(unit tensor, slot) of a synthesized expert Linear `...mlp.experts.<e>.w1|w3|w2` (or its checkpoint name)."""
        return self.expert_of.get(moe_calibration.checkpoint_name(name))

    def _unit_slice(self, unit: str, e: int, t: int, R: int, C: int, device) -> torch.Tensor:
        """Slot e of the unit's level of type t as a flat byte view: the device buffer [E, R, C / block * type_size] is
        allocated, and the level registered with its 3-D shape, when the first slice is asked for."""
        from .gguf_writer import GGML_QUANT_SIZES
        bs, ts = GGML_QUANT_SIZES[int(t)]
        rec = self.units.get((unit, int(t)))
        cuda = torch.device(device).type == "cuda"
        if rec is None:
            buf = torch.empty((self.n_experts, R, C // bs * ts), dtype=torch.uint8, device=device)
            born = None
            if cuda:  # where, and after what, the buffer came to be: see the rule below
                born = (torch.cuda.current_stream(device), torch.cuda.Event())
                born[1].record(born[0])
            rec = self.units[(unit, int(t))] = [buf, set(), self.writer.register(unit, (self.n_experts, R, C), int(t)), born]
        buf, filled, _, born = rec
        # THE RULE for a buffer shared by the lanes of a block.  It is allocated under whichever lane asks first, and the
        # caching allocator may hand that lane a block whose earlier tenant (a working copy, a workspace of an earlier walk)
        # is still in use by kernels queued on that SAME stream -- safe there, in stream order, and nowhere else.  So a lane
        # on another stream waits for the event recorded on the allocating stream at allocation before its first write, and
        # the buffer is marked as used on that lane's stream so that it is not reused under it once it is dropped.
        if born is not None:
            here = torch.cuda.current_stream(device)
            if here != born[0]:
                here.wait_event(born[1])
                buf.record_stream(here)
        if tuple(buf.shape[1:]) != (R, C // bs * ts) or e in filled or not 0 <= e < self.n_experts:
            raise RuntimeError(f"level_db: slot {e} of {unit} (type {int(t)}) is out of range, filled twice or of another shape "
                               f"than {tuple(buf.shape)}")
        filled.add(e)
        return buf[e].view(-1)

    def _pack_expert_walk(self, stacked, bands, members, tensors, slots):
        """pack_walk for a walk with expert bands: band k goes straight into slot e of its unit's buffer (caller-owned outs
        of ONE gq_pack_bands launch; with rows a multiple of 64 every slice is 16-byte aligned).  No rotary row gather, no
        per-expert temporary.  A stale band, and a band of a plain Linear in the same walk, get a buffer of their own."""
        from .gguf_writer import GGML_QUANT_SIZES
        q = stacked[0]
        dev, C = q.device, q.shape[1]
        outs, srcs, r0 = [], [], 0
        for (r1, t), mem, tensor, slot in zip(bands, members, tensors, slots):
            if (r1 - r0) % 64:
                raise NotImplementedError(f"level_db: a band of {r1 - r0} rows next to an expert band (multiples of 64 only)")
            if slot is not None:
                outs.append(self._unit_slice(slot[0], slot[1], int(t), r1 - r0, C, dev))
                srcs.append(None)
            else:
                outs.append(torch.empty((r1 - r0) * (C // 256) * GGML_QUANT_SIZES[int(t)][1], dtype=torch.uint8, device=dev))
                srcs.append(self._row_src(tensor, r1 - r0, dev) if tensor is not None else None)
            r0 = r1
        outs = _ops.pack_bands(stacked, bands, outs, srcs)
        r0 = 0
        for (r1, t), mem, tensor, slot, out in zip(bands, members, tensors, slots, outs):
            if slot is None and tensor is not None:
                path = self.writer.register(tensor, (r1 - r0, C), int(t))
                self.items.append((path, RAW_BYTES, (out.view(-1),)))
                self.packed.add(mem[0])
            r0 = r1
        return outs

    def _encode_iq4_expert(self, slot, weight: torch.Tensor, importance: Optional[torch.Tensor]) -> List[torch.Tensor]:
        """encode_iq4 for one expert matrix: each type's bytes go into slot e of the unit's buffer."""
        from .gguf_writer import GGML_QUANT_SIZES
        w = weight.detach()
        if w.dim() != 2 or w.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise NotImplementedError(f"level_db_iq4: {slot[0]} has a {w.dtype} expert weight of shape {tuple(w.shape)}")
        w = w.contiguous()
        outs = []
        for t in self.iq4:
            if w.shape[1] % GGML_QUANT_SIZES[t][0]:
                continue
            out = self._unit_slice(slot[0], slot[1], t, w.shape[0], w.shape[1], w.device)
            outs.append(_ops.quantize_iq4(w, t, importance, None, out=out))
        return outs

    def end_group(self) -> None:
        """The block's _quant_group is over: every started (unit, level) must hold all E slices -- a hole raises -- and its
        bytes are queued for the saver."""
        for (unit, t), (buf, filled, path, _) in self.units.items():
            if len(filled) != self.n_experts:
                missing = sorted(set(range(self.n_experts)) - filled)
                raise RuntimeError(f"level_db: {unit} (type {t}) was started but slots {missing} of {self.n_experts} were never "
                                   f"filled: a unit is written whole or not at all")
            self.items.append((path, RAW_BYTES, (buf.view(-1),)))
            self.packed.add(unit)
        self.units = {}

    def encode_iq4(self, name: str, weight: torch.Tensor, importance: Optional[torch.Tensor]) -> List[torch.Tensor]:
        """The IQ4 levels of HF module `name` from its unmodified `weight` [R, C] on the current stream: one gq_quantize_iq4
        launch per type, the bytes booked and queued like a walk's.  Nothing for a module the database does not hold."""
        from .gguf_writer import GGML_QUANT_SIZES
        slot = self._slot_of(name)
        if slot is not None and self.iq4:
            return self._encode_iq4_expert(slot, weight, importance)
        tensor = self.tensor_of.get(name)
        if tensor is None or not self.iq4:
            return []
        w = weight.detach()
        if w.dim() != 2 or w.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise NotImplementedError(f"level_db_iq4: {name} has a {w.dtype} weight of shape {tuple(w.shape)}")
        w = w.contiguous()
        rows = self._row_src(tensor, w.shape[0], w.device)
        outs = []
        for t in self.iq4:
            if w.shape[1] % GGML_QUANT_SIZES[t][0]:
                continue  # (rows that are no multiple of the type's block: the tensor has no such level)
            blocks = _ops.quantize_iq4(w, t, importance, rows)
            path = self.writer.register(tensor, tuple(w.shape), t)
            self.items.append((path, RAW_BYTES, (blocks.view(-1),)))
            outs.append(blocks)
        return outs

    def before_levels(self, name: str, handle) -> List[torch.Tensor]:
        """BlockSchedule.quantize_levels' `before`: handle.H is the accumulated Hessian (undamped), handle.layer.weight the
        block's unmodified weight."""
        imp = None
        if self.iq4_importance == "hessian":
            imp = handle.H.diagonal().contiguous()  # (a copy: _prepare damps H in place later on this stream)
        if self.iq4_method == "gptq":  # the levels are built behind the walk, from the factorisation: after_levels
            self._iq4_imp[name] = imp
            return [imp] if imp is not None else []
        return self.encode_iq4(name, handle.layer.weight, imp) + ([imp] if imp is not None else [])

    def after_levels(self, name: str, handle, results) -> List[torch.Tensor]:
        """BlockSchedule.quantize_levels' `extra` under iq4_method "gptq": handle._last_U / _last_cf are the Linear's
        factorisation and column flags, handle.layer.weight still the block's unmodified weight.  Per type a fresh working
        copy with the dead columns of the first one (as GPTQ.compute_levels makes its later levels'), one walk, one pack."""
        imp = self._iq4_imp.pop(name, None)
        tensor, slot = self.tensor_of.get(name), self._slot_of(name)
        if (tensor is None and slot is None) or not self.iq4:
            return []
        rows = self._row_src(tensor, handle.d_row, handle.W_device) if slot is None else None
        outs = []
        for t in self.iq4:
            if handle.d_col % 256:
                continue  # (the walk's rule; such a tensor has no K-quant level either)
            handle.make_working_copy()
            _ops.w_prepare(handle._last_cf, handle.W)
            q, d, ls, _ = _ops.gptq_quantize_iq4(handle.W, handle._last_U, t, handle.block_size, imp)
            if slot is not None:  # packed straight into slot e of the unit's buffer
                blocks = _ops.pack_iq4(t, q, d, ls, None,
                                       out=self._unit_slice(slot[0], slot[1], t, handle.d_row, handle.d_col, q.device))
            else:
                blocks = _ops.pack_iq4(t, q, d, ls, rows)
                path = self.writer.register(tensor, (handle.d_row, handle.d_col), t)
                self.items.append((path, RAW_BYTES, (blocks.view(-1),)))
            outs += [blocks, handle.W]
        return outs

    def take(self) -> List[tuple]:
        items, self.items = self.items, []
        return items

    def finish(self) -> str:
        """Every level file is on disk (the saver is closed): the key/value data, the plain tensors, close()."""
        from .gguf_writer import GGMLType, GGUFWriter, kv_records
        from .pack_gptq_into_gguf import (FTYPE, SKIPPED_HF_TENSORS, add_model_metadata, iter_hf_entries, permute, plain_tensor,
                                          rope_freqs_llama3)
        w = self.writer
        kv = GGUFWriter(None, self.gguf_arch)  # collects the key/value data; never written
        add_model_metadata(kv, self.hp, self.dir_model, FTYPE["f16"][0], self.total_params, self.expert_params, self.vocab)
        w.set_metadata(kv_records(kv.kv))

        def plain(tensor, data):
            arr, raw = plain_tensor(tensor, data, "f16")
            arr = np.ascontiguousarray(arr)
            w.add_level(tensor, arr.shape, raw if raw is not None else (GGMLType.F32 if arr.dtype == np.float32 else GGMLType.F16), arr)

        if self.rope_type == "llama3":
            plain("rope_freqs.weight", rope_freqs_llama3(self.hp))
        pending: Dict[str, dict] = {}  # unit tensor -> {slot: the checkpoint's expert matrix}, until all E are read
        for name, _, get in iter_hf_entries(self.dir_model):
            base = name.removesuffix(".weight")
            if name.endswith(SKIPPED_HF_TENSORS):
                continue
            if base in self.expert_of:
                unit, e = self.expert_of[base]
                if unit in self.packed and not self.q8_0:
                    continue
                got = pending.setdefault(unit, {})
                got[e] = get()
                if len(got) < self.n_experts:
                    continue
                x = torch.stack([got[i] for i in range(self.n_experts)], dim=0)  # [E, R, C], as the converter stacks them
                del pending[unit]
                if unit in self.packed:  # the 8.5-bit level of a packed unit: [E R, C] through ONE gq_quantize_q8_0
                    x = x.to(self.device)
                    if x.dtype not in (torch.float32, torch.float16, torch.bfloat16):
                        x = x.float()
                    blocks = _ops.quantize_q8_0(x.view(-1, x.shape[-1]).contiguous(), None)
                    w.add_level(unit, tuple(x.shape), GGMLType.Q8_0, blocks.view(x.shape[0], x.shape[1], -1).cpu().numpy())
                else:
                    plain(unit, x)
                continue
            if base in self.packed:
                if self.q8_0:  # the 8.5-bit level: RTN of the checkpoint's own weights, registered after the K-quant levels
                    x = get().to(self.device)
                    if x.dtype not in (torch.float32, torch.float16, torch.bfloat16):
                        x = x.float()
                    tensor = self.tensor_of[base]
                    blocks = _ops.quantize_q8_0(x, self._row_src(tensor, x.shape[0], x.device))
                    w.add_level(tensor, tuple(x.shape), GGMLType.Q8_0, blocks.cpu().numpy())
                continue
            data = get()
            if self.gguf_arch == "llama" and name.endswith("q_proj.weight"):
                data = permute(data, self.n_head, self.n_head)
            elif self.gguf_arch == "llama" and name.endswith("k_proj.weight"):
                data = permute(data, self.n_head, self.n_kv)
            plain(self.tensor_of[base], data)
        return w.close()


class Quantizer:
    def __init__(self, model: nn.Module, data_loader: Iterable, quantizable_modules: str,
                 quantizer_kwargs: Dict[str, Any], pre_block_modules: List[str], post_block_modules: List[str],
                 block_modules: str, save_dir: str, quant_non_block_modules: bool = False,
                 device: Optional[torch.device] = None, cpu_offload_modules: bool = False,
                 cpu_offload_activations: bool = False, verbose: bool = False, non_block_fp32: bool = False,
                 calibration_batch: int = 1, fused_forward="exact", interrupt_forward1: bool = True) -> None:
        self.model = model
        self.data_loader = data_loader
        self.quantizable_modules = quantizable_modules
        self.quantizer_kwargs = quantizer_kwargs
        self.pre_block_modules = pre_block_modules
        self.post_block_modules = post_block_modules
        self.block_modules = block_modules
        self.device = device
        self.cpu_offload_modules = cpu_offload_modules
        self.cpu_offload_activations = cpu_offload_activations
        self.quant_non_block_modules = quant_non_block_modules
        self.verbose = verbose
        self.save_dir = save_dir
        self.non_block_fp32 = non_block_fp32
        # beyond the reference (which runs one calibration sample per block forward, quantizer.py:150-151): samples
        # per block forward.  Same Hessians in exact arithmetic (GPTQ.update weighs a batch by its size,
        # gptq.py:86-112); one Llama-3-8B layer forward takes 0.91 instead of 1.16 ms per sequence at 4.
        self.calibration_batch = max(1, int(calibration_batch))
        # forward #1 of a block (quantizer.py:150-151) only feeds the Hessian hooks, its output is discarded: stop it at the
        # last hooked Linear (learned on the block's first sample; BlockSchedule.pre_hook).  Same Hessians, same bytes saved.
        # The same switch drops forward #2 of the LAST block, whose outputs nothing reads.
        self.interrupt_forward1 = bool(interrupt_forward1)
        # beyond the reference (which runs the HF eager modules, quantizer.py:293): HIP kernels for the elementwise
        # modules of the block forward (forward_fused.py).  "exact" (default): rotary embedding, SwiGLU and RMSNorm, each
        # bit-identical to HF eager (RMSNorm verified at run time on this PyTorch before it is trusted) -- the saved
        # tensors do not change; "all" / True: RMSNorm's free-order kernel (<= 2 ulp) where the exact one is not
        # verified; "off" / False: none.  GQ_FUSED_FORWARD=off|exact|all overrides (A/B runs).
        self.fused_forward = level_of(os.environ.get("GQ_FUSED_FORWARD", fused_forward))

    # ------------------------------------------------------------------ walk
    @torch.no_grad()
    def quantize_levels(self, levels, propagate, level_db: Optional[str] = None, trees: bool = True,
                        level_db_model: Optional[str] = None, level_db_vocab: bool = True, level_db_q8_0: bool = False,
                        level_db_iq4=(), level_db_iq4_importance: str = "hessian", level_db_iq4_method: str = "rtn",
                        fused_experts: bool = False) -> None:
        """The level database in one pass: every quantizable module at every level of `levels`, one ordinary tree per level
        under <save_dir>/<LEVEL>/ (level_tree_name; same schema, same writer as quantize()).  The calibration forwards, the
        Hessians, the factorisations and the column walk are those of ONE run (BlockSchedule.quantize_levels).
        `propagate`: the level whose dequantized weights replace the model's -- every later block is calibrated on what an
        ordinary all-<propagate> run feeds it, so that level's tree and the model afterwards are that run's -- or None:
        the model stays untouched and every block is calibrated on full-precision activations.  With
        quant_non_block_modules, embed / lm_head are RTN-quantized per level (what --default_bit_width LEVEL writes).

        `level_db`: also write the level database there (a directory that does not exist yet) -- what converting every
        level's tree and splitting the files with --exact leaves, packed on the GPU with one gq_pack_bands launch per walk
        (_LevelDbSink; level_db.py lists how it differs from a split).  `level_db_model`: the model's directory (default: the
        model's own name_or_path, which must be a local directory), `level_db_vocab`: write the tokenizer keys, as
        convert(vocab=...).  `trees=False` (with level_db): the per-level trees are not written.  `level_db_q8_0` (with
        level_db): every tensor that has K-quant levels also gets the 8.5-bit level 8.5-Q8_0.pth, round-to-nearest of its
        unmodified weights.  `level_db_iq4` (with level_db; names out of "IQ4_XS", "IQ4_NL"): it also gets the levels
        4.25-IQ4_XS.pth / 4.56-IQ4_NL.pth, encoded from its unmodified weights with the diagonal of its calibration Hessian as
        the importance of a column (`level_db_iq4_importance` "hessian"; "none": unweighted) -- _LevelDbSink.
        `level_db_iq4_method` "rtn" (default): round-to-nearest; "gptq": the IQ4 levels of every Linear come out of GPTQ's
        column walk on the IQ4 grid with the same importance (gq_gptq_quantize_iq4; embed / lm_head stay round-to-nearest).
        `fused_experts=True`: fused experts (transformers 5.x MixtralExperts) that quantizable_modules names are walked as in
        quantize() -- moe_calibration.CalibExperts per block, hooks on the synthesized experts.<e>.w1 / w3 / w2 Linears, the
        propagated level written back through the views; every tree goes under the checkpoint's name
        (<save_dir>/<LEVEL>/model.layers.N.block_sparse_moe.experts.<e>.w{1,2,3}), an expert no calibration token reaches has
        H = I (its K-quant levels are round-to-nearest), and the database holds the stacked units.  Without it such a model
        is refused, by name.
        Everything is refused before any work; a failed run leaves no database."""
        levels, propagate = check_levels(levels, propagate)
        if dist_utils.get_world_size() > 1:
            raise NotImplementedError("quantize_levels runs on one rank (multi-rank level builds are not built)")
        if self.quantizer_kwargs.get("act_order") or self.quantizer_kwargs.get("static_groups"):
            raise ValueError("quantize_levels: act_order / static_groups have no level build")
        if level_db is None and not trees:
            raise ValueError("quantize_levels: trees=False needs level_db (nothing would be written)")
        if level_db is None and level_db_q8_0:
            raise ValueError("quantize_levels: level_db_q8_0 needs level_db (the Q8_0 level is a level of the database)")
        if level_db is None and level_db_iq4:
            raise ValueError("quantize_levels: level_db_iq4 needs level_db (the IQ4 levels are levels of the database)")
        check_iq4_levels(level_db_iq4, level_db_iq4_importance, level_db_iq4_method)
        fused = moe_calibration.named_fused_experts(self.model, self.block_modules + ".", self.quantizable_modules)
        if fused and not fused_experts:
            raise NotImplementedError(f"quantize_levels: {fused[0][0]} ({type(fused[0][1]).__name__}) keeps fused experts that "
                                      "quantizable_modules names; their level build is opt-in: pass fused_experts=True "
                                      "(quant.py --level_fused_experts)")
        for name, layer in fused:  # refused before any work, as install() would per block
            why = moe_calibration.why_not_adaptable(layer)
            if why:
                raise NotImplementedError(f"{name} ({type(layer).__name__}): --quantizable_modules names its experts, but {why}")
        sink = None
        if level_db is not None:
            if os.environ.get("GQ_SAVE_SKIP") == "1":
                raise ValueError("quantize_levels: GQ_SAVE_SKIP=1 writes no files, a level database cannot be completed")
            sink = _LevelDbSink(level_db, level_db_model or getattr(self.model.config, "_name_or_path", None), level_db_vocab,
                                q8_0=level_db_q8_0, iq4=level_db_iq4, iq4_importance=level_db_iq4_importance,
                                iq4_method=level_db_iq4_method)
        self._levels, self._level_src, self._level_sink, self._level_trees = (levels, propagate), {}, sink, bool(trees)
        try:
            self.quantize({})
            if sink is not None:
                sink.finish()
        except BaseException:
            if sink is not None:
                sink.writer.abort()
            raise
        finally:
            self._levels, self._level_src, self._level_sink, self._level_trees = None, {}, None, True

    @torch.no_grad()
    def quantize(self, quant_config: Dict[str, GGMLQuantizationType]) -> None:
        device = self.device or next(self.model.parameters()).device
        self._save_index = -1
        self._saver = _Saver(self.save_dir, sync=False)
        if os.environ.get("GQ_SAVE_SKIP") != "1":
            self._saver.warm_up(device)
        self._saved_names: List[str] = []
        self._calib_experts: list = []          # moe_calibration.install()'s records of the block in work
        self._tree_names: Dict[str, str] = {}   # synthesized expert Linear -> the checkpoint's name its tree is written under
        try:
            reset_verdicts()  # every run re-verifies the forward kernels on its own first inputs
            moe_calibration.reset_verdicts()
            with fused_forward(self.fused_forward if torch.device(device).type == "cuda" else "off") as patched:
                self._fused_modules = patched
                self._quantize(quant_config, device)
        finally:
            moe_calibration.restore(self._calib_experts)  # (a run that raised inside a block: the model gets its own modules back)
            BlockSchedule.discard_checks()  # nothing of this run may leak into the next Quantizer of the process
            t0 = time.perf_counter()
            self._saver.close()
            dist_utils.barrier()  # every rank's files are on disk
            self._check_saved_files()
            if getattr(self, "_phases", None) is not None:
                self._phases.host["save_tail"] = time.perf_counter() - t0
                self.timing = self._phases.result()
                if torch.device(device).type == "cuda":
                    ms = torch.cuda.memory_stats(device)
                    self.timing["allocator"] = {"device_allocs": ms["num_device_alloc"], "segments": ms["segment.all.current"],
                                                "reserved_GiB": round(ms["reserved_bytes.all.peak"] / 2**30, 1),
                                                "active_peak_GiB": round(ms["active_bytes.all.peak"] / 2**30, 1)}
                self.timing["saver_copy_thread_busy_s"] = round(self._saver.busy_s, 4)
                self.timing["saver_close_split_s"] = getattr(self._saver, "close_split", None)
                self.timing["saver_writer_process_busy_s"] = round(getattr(self._saver, "writer_busy_s", 0.0), 4)

    def _quantize(self, quant_config: Dict[str, GGMLQuantizationType], device) -> None:
        ph = self._phases = _Phases(device)
        blocks = self.model.get_submodule(self.block_modules)
        pre_blocks = [(n, self.model.get_submodule(n)) for n in self.pre_block_modules]
        post_blocks = [(n, self.model.get_submodule(n)) for n in self.post_block_modules]
        blocks[0] = blocks[0].to(device)
        for _, m in pre_blocks:
            m.to(device)
        use_cache = getattr(self.model.config, "use_cache", None)
        if use_cache is not None:
            self.model.config.use_cache = False
        # capture the inputs of block 0 for every calibration sample (quantizer.py:78-89)
        blocks[0] = InputCollector(blocks[0], cpu_offload=self.cpu_offload_activations)
        for inp_args, inp_kwargs in self.data_loader:
            try:
                self.model(*_to(inp_args, device=device), **_to(inp_kwargs, device=device))
            except ForwardInterrupt:
                pass
        input_args, input_kwargs = blocks[0].input_args, blocks[0].input_kwargs
        blocks[0] = blocks[0].module
        if self.calibration_batch > 1:
            input_args, input_kwargs = _batch_block_inputs(input_args, input_kwargs, self.calibration_batch)
        dist_utils.barrier()
        ph.mark("capture")

        if self.quant_non_block_modules:
            for name, module in pre_blocks:
                self._quant_and_save_non_block(name, module.to(device), quant_config)
        if self.cpu_offload_modules:
            for _, m in pre_blocks:
                m.cpu()
        ph.mark("rtn_pre")
        # Where the post-block modules (lm_head) are quantized.  Their RTN reads nothing the block loop writes -- same tensors
        # and files wherever it runs (a tied lm_head still sees embed_tokens' RTN first) -- but lm_head's data.pth (657 MB for
        # Llama-3-8B: 0.6 s of clone + torch.save in the writer) is the tail of the run when it comes last, as in the
        # reference (quantizer.py:181-198).  Default: right before the LAST block, so that the file is written under that
        # block's work (save tail 0.65 -> 0.3 s).  GQ_POST_BLOCKS=last: the reference's place; =early: before the block loop
        # (same gain; with two staging slots 2 of 5 such runs fell into the slow mode described at _Saver.put_many).
        post_where = os.environ.get("GQ_POST_BLOCKS", "before_last_block") if self.quant_non_block_modules else "none"
        if post_where not in ("none", "early", "before_last_block", "last"):
            raise ValueError(f"GQ_POST_BLOCKS={post_where!r}: expected early / before_last_block / last")
        post_early = post_where == "early"
        if post_early:
            for name, module in post_blocks:
                self._quant_and_save_non_block(name, module.to(device), quant_config)
            ph.mark("rtn_post")

        for block_id, block in enumerate(blocks):
            if post_where == "before_last_block" and block_id == len(blocks) - 1:
                for name, module in post_blocks:
                    self._quant_and_save_non_block(name, module.to(device), quant_config)
                ph.mark("rtn_post")
            if self.verbose:
                dist_utils.print_on_main(f"Processing {self.block_modules} {block_id}/{len(blocks)}.")
            block = block.to(device)
            prefix = f"{self.block_modules}.{block_id}."
            # fused experts (transformers 5.x MixtralExperts) that the regex names: a stand-in with one nn.Linear per expert
            # matrix, views of the fused storage, for this block's two forwards and its column walks (moe_calibration.py)
            routed = torch.device(device).type == "cuda" and self.fused_forward in moe_calibration.ROUTED_LEVELS
            self._calib_experts += moe_calibration.install(self.model, prefix, self.quantizable_modules,
                                                           "routed" if routed else "loop")
            for _, _, original, name in self._calib_experts:
                for n in moe_calibration.synthesized_names(name, original.down_proj.shape[0]):
                    self._tree_names[n] = moe_calibration.checkpoint_name(n)
            layers = select_layers(self.model, prefix, self.quantizable_modules, LINEAR_LAYERS)
            handles, hooks = self._prepare_hooks_and_handles(layers, block)
            sched = self._schedule
            for a, kw in zip(input_args, input_kwargs):  # forward #1: Hessians (quantizer.py:150-151)
                try:
                    block(*_to(a, device=device), **_to(kw, device=device))
                except ForwardInterrupt:  # every hooked Linear has been fed; the reference discards the output anyway
                    pass
                sched.sample_done()  # grouped SYRK launches once the buffers hold flush_tokens tokens
            for h in hooks.values():
                h.remove()
            ph.mark("forward1+H")
            self._quant_group(handles, quant_config)
            ph.mark("quant_group")
            # forward #2: propagate (quantizer.py:161-172).  After the LAST block nothing reads the propagated activations (the
            # post-block modules are quantized from their weights alone, quantizer.py:181-198): that forward is not run
            dead = self.interrupt_forward1 and block_id == len(blocks) - 1
            for a, kw in (() if dead else zip(input_args, input_kwargs)):
                out = _first(block(*_to(a, device=device), **_to(kw, device=device)))
                if self.cpu_offload_activations:
                    out = out.cpu()
                if len(a) > 0:
                    a[0].data = out
                elif "hidden_states" in kw:
                    kw["hidden_states"] = out
                else:
                    raise ValueError("Unsupported block input format.")
            moe_calibration.restore(self._calib_experts)  # the block's own modules are back, holding the quantized weights
            if self.cpu_offload_modules:
                block.cpu()
            del handles, hooks, sched
            self._schedule = None
            # reused-factorisation flags: this block's go to the host behind an event, earlier blocks' are read if
            # they have arrived -- a mismatch (the host-side pre-check makes it unlikely) stops the run at once
            # instead of after the whole model, and the host never waits for the device here
            BlockSchedule.verify(wait=False)
            ph.mark("forward2")
            if "blocks" in os.environ.get("GQ_TRACE", ""):  # measurement knob: per-block wall time (synchronises)
                torch.cuda.synchronize()
                now = time.perf_counter()
                ms = torch.cuda.memory_stats(device)
                print(f"[gq] block {block_id}: {1e3 * (now - getattr(self, '_t_block', now)):.1f} ms "
                      f"(saver queue {self._saver.q.qsize()}; reserved {ms['reserved_bytes.all.current'] >> 20} MiB in "
                      f"{ms['segment.all.current']} segments, {ms['num_device_alloc']} device allocs, "
                      f"active {ms['active_bytes.all.current'] >> 20} MiB)", file=sys.stderr)
                self._t_block = now

        if post_where == "last" or (post_where == "before_last_block" and len(blocks) == 0):
            for name, module in post_blocks:
                self._quant_and_save_non_block(name, module.to(device), quant_config)
        if self.quant_non_block_modules:  # wherever they ran, they ran: the packer would silently write a missing one as f16
            saved = {n.rsplit("/", 1)[-1] for n in self._saved_names}  # (a level build saves <LEVEL>/<module>)
            sink = getattr(self, "_level_sink", None)
            if sink is not None and not getattr(self, "_level_trees", True):  # no trees: what the database holds instead, and
                saved |= sink.packed | {n for n, _ in pre_blocks + post_blocks if n not in sink.tensor_of}  # (a tied lm_head)
            missing = [n for n, _ in pre_blocks + post_blocks if n not in saved]
            assert not missing, f"non-block modules never quantized: {missing}"
        if use_cache is not None:
            self.model.config.use_cache = use_cache
        BlockSchedule.verify()  # whatever is still on its way
        ph.mark("rtn_post")
        dist_utils.barrier()

    # --------------------------------------------------------- hooks / handles
    def _create_handle(self, layer, name: str = "") -> GPTQ:
        # MoE expert Linears ("...experts.<e>.w1"): the router may send them no calibration token at all, and a
        # data-dependent number per rank -- the handle then falls back to H = I and reduces H sample-weighted
        # (the reference asserts, gptq.py:126, and averages unweighted)
        return GPTQ(layer, allow_no_samples=".experts." in f".{name}.", **self.quantizer_kwargs)

    def _prepare_hooks_and_handles(self, layers: Dict[str, nn.Module], block: Optional[nn.Module] = None):
        """reference quantizer.py:221-239; the hook body lives in BlockSchedule.feed.  `block`: its Linears outside `layers`
        get a flag-only pre-hook, so that forward #1 is interrupted only when the last Linear to run is a hooked one."""
        self._schedule = BlockSchedule(layers, self._create_handle, verbose=self.verbose)
        # forward PRE-hooks: same inp[0] as the reference's forward hook (quantizer.py:229), available before the Linear's
        # GEMM, so that forward #1 can stop at the last hooked Linear (BlockSchedule.pre_hook)
        hooks = {name: layer.register_forward_pre_hook(self._schedule.pre_hook(name, self.interrupt_forward1))
                 for name, layer in layers.items()}
        if block is not None and self.interrupt_forward1:
            hooked = {id(l) for l in layers.values()}
            for i, m in enumerate(block.modules()):
                if isinstance(m, tuple(LINEAR_LAYERS)) and id(m) not in hooked:
                    hooks[f"<unhooked {i}>"] = m.register_forward_pre_hook(self._schedule.other_pre_hook())
        return self._schedule.handles, hooks

    # ------------------------------------------------------------- quantize
    def _check_saved_files(self) -> None:
        """The data.pth files are dealt to the ranks; all of them must end up in ONE directory (the packer treats a
        missing module as unquantized and would silently write it as f16).  After the barrier rank 0 looks: on a
        multi-node run with a node-local save_dir this is where it shows."""
        if not dist_utils.is_main() or os.environ.get("GQ_SAVE_SKIP") == "1" or sys.exc_info()[0] is not None:
            return
        missing = [n for n in self._saved_names if not os.path.isfile(os.path.join(self.save_dir, n, "data.pth"))]
        if missing:
            raise RuntimeError(f"{len(missing)} of {len(self._saved_names)} data.pth files are not in {self.save_dir} "
                               f"(first: {missing[0]}): save_dir must be shared by all ranks")

    def _save(self, name, q_type, qweight, d, s, dmin, m, defer: bool = False):
        self._saved_names.append(name)
        # every rank holds every result after the exchange: the files are dealt round-robin to the ranks of the
        # node (the reference lets every rank write every file, quantizer.py:267-275), so that the device-to-host
        # copies and the zip/CRC work of torch.save -- ~1 GB/s per writer, 8.7 GB for Llama-3-8B -- scale with
        # the ranks instead of serialising on rank 0 next to an 8x shorter compute phase
        self._save_index = getattr(self, "_save_index", -1) + 1
        if self._save_index % dist_utils.get_world_size() != dist_utils.get_rank() or os.environ.get("GQ_SAVE_SKIP") == "1":
            return  # (GQ_SAVE_SKIP: measurement knob -- how much of the wall time the writer costs)
        if defer:
            return (name, q_type, (qweight, d, s, dmin, m))
        self._saver.put(name, q_type, (qweight, d, s, dmin, m))

    def _quant_group(self, handles: Dict[str, GPTQ], quant_config: Dict[str, GGMLQuantizationType]):
        """reference quantizer.py:241-275: quantize every handle, write the dequantized weight back, save."""
        qtypes = {n: quant_config.get(n.split(".")[-1], GGMLQuantizationType.Q4_K) for n in handles}
        sched = self._schedule
        assert sched is not None and sched.handles is handles
        batch = []
        if getattr(self, "_levels", None) is not None:
            levels, propagate = self._levels
            sink = getattr(self, "_level_sink", None)
            before = sink.before_levels if sink is not None and sink.iq4 else None
            after = sink.after_levels if before is not None and sink.iq4_method == "gptq" else None
            for n, per_level in sched.quantize_levels(levels, propagate, extra=after, pack=sink.pack_walk if sink else None,
                                                      before=before).items():
                for t in levels if getattr(self, "_level_trees", True) else ():
                    item = self._save(level_tree_name(t, self._tree_names.get(n, n)), t, *per_level[t], defer=True)
                    if item is not None:
                        batch.append(item)
            if sink is not None:
                sink.end_group()  # (a unit with a hole raises here)
            if sink is not None and os.environ.get("GQ_SAVE_SKIP") != "1":
                batch.extend(sink.take())
            self._saver.put_many(batch)
            self.schedule_stats = sched.stats
            return
        tree = getattr(self, "_tree_names", {})
        for n, res in sched.quantize(qtypes, writeback=True).items():
            item = self._save(tree.get(n, n), qtypes[n], *res, defer=True)
            if item is not None:
                batch.append(item)
        self._saver.put_many(batch)  # the block's files travel in one staging slot
        self.schedule_stats = sched.stats

    def _quant_non_block_module(self, w: torch.Tensor, q_type: GGMLQuantizationType):
        """RTN for embed / lm_head (reference quantizer.py:278-330)."""
        kw = self.quantizer_kwargs
        # fp16 / bf16 weights: the reference runs make_*quants in the model dtype (quantizer.py:109,195);
        # gq_rtn_quantize reproduces that per-op rounding.  non_block_fp32 opts into an fp32 search instead.
        if w.dtype != torch.float32 and self.non_block_fp32:
            w = w.float()
        # quant_scale is forwarded like the reference does (quantizer.py:293-295; grid / maxshrink stay at
        # Quantizer.configure's defaults there, quant_utils.py:65-66).  make_k_quants ignores it.
        quant_scale = getattr(kw.get("quant_scale", "absmax"), "value", kw.get("quant_scale", "absmax"))
        if quant_scale == "mse" and w.dtype != torch.float32 and \
                q_type in (GGMLQuantizationType.Q3_K, GGMLQuantizationType.Q6_K):
            # the reference cannot run this combination: make_quants builds min_loss in fp32 (quant_utils.py:165) and
            # index_puts the model-dtype loss into it (:187) -> RuntimeError; same error class here, before any work
            raise RuntimeError(
                f"quant_scale='mse' on a {w.dtype} weight with {q_type.name}: the reference raises here (Index put "
                "requires the source and destination dtypes match, quant_utils.py:187). Use --dtype float32 or "
                "--non_block_fp32.")
        return _ops.rtn_quantize(w.contiguous(), int(q_type), kw.get("rmin", -1.0), kw.get("rdelta", 0.1),
                                 kw.get("nstep", 20), quant_scale=quant_scale)

    def _quant_and_save_non_block(self, name, module, quant_config):
        if self.verbose:
            dist_utils.print_on_main(f"Processing {name}.")
        if getattr(self, "_levels", None) is not None:
            return self._quant_and_save_non_block_levels(name, module)
        q_type = quant_config.get(name.split(".")[-1], GGMLQuantizationType.Q6_K)  # quantizer.py:107,192
        qweight, d, s, dmin, m = self._quant_non_block_module(module.weight, q_type)
        module.weight.data = dequantize_linear_weight(q_type, qweight, d, s, dmin, m,
                                                      out_dtype=module.weight.data.dtype)
        self._save(name, q_type, qweight, d, s, dmin, m)

    def _quant_and_save_non_block_levels(self, name, module):
        """embed / lm_head of a level build: RTN per level, each what an all-<level> run writes; only the propagated level is
        written back.  A module whose weight an earlier non-block module already went through (a tied lm_head) sees, per
        level, that level's dequantized weight -- as it does in the all-<level> run, where embed_tokens' write-back comes
        first."""
        levels, propagate = self._levels
        key = id(module.weight)
        tied = key in self._level_src
        src = self._level_src.setdefault(key, module.weight.data)  # the weight before any write-back (kept alive here)
        back = None
        sink = getattr(self, "_level_sink", None)
        if sink is not None and sink.iq4:  # no Hessian here: the IQ4 levels are unweighted, and come before the K-quant levels
            sink.encode_iq4(name, src, None)
            self._saver.put_many(sink.take())
        for t in levels:
            w = src
            if tied:
                w = dequantize_linear_weight(t, *self._quant_non_block_module(src, t), out_dtype=src.dtype)
            res = self._quant_non_block_module(w, t)
            if t == propagate:
                back = dequantize_linear_weight(t, *res, out_dtype=module.weight.data.dtype)
            if getattr(self, "_level_trees", True):
                self._save(level_tree_name(t, name), t, *res)
            sink = getattr(self, "_level_sink", None)
            if sink is not None:
                sink.pack_walk(res, [(res[0].shape[0], int(t))], [(name, t)])
                self._saver.put_many(sink.take())
        if back is not None:
            module.weight.data = back
