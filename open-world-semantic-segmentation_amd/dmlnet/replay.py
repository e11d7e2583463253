"""Running a built plan: refresh the weight copies when the masters changed, then replay the op lists."""
# Replay is one C call per contiguous run of ops (dml_plan_run), or op by op from Python.
import ctypes as C

import torch

from . import _lib
from .launch_list import NativeList


class Replay:
    """mixed into dmlnet.engine.Plan beside PlanPieces, whose op lists and bookkeeping it reads"""

    def refresh_weights(self, stream, overlap=False):
        """compute copies / fp16 planes of the weights after the masters changed.  overlap (training forward): the copies of layer2 and
        everything behind it are made on the engine's side stream while the stem and layer1 run (their own few copies first, on the
        caller's stream); run_forward waits for the side stream's event at Plan.prep_cut.  0.5 ms of launches that only depend on the
        optimizer step leave the forward's critical path."""
        st = self.e.store
        key = (st.version, sum(p._version for p in st.params))
        if key == self.prepped_version:
            return
        for fn in self.pre_prep:
            fn()
        self.prep_event = None
        if self.prep_table is None:
            self.prep_table = []
            for dt in sorted({e[7] for e in self.prep}):          # one table launch per storage type present in the plan
                ent = [e for e in self.prep if e[7] == dt]
                arr = (_lib.PrepDesc * len(ent))()
                for i, (src, w, wt, N, RS, Cm, Cp, _, w_tiled, wt_tiled) in enumerate(ent):
                    arr[i] = _lib.PrepDesc(src, w, wt or None, N, RS, Cm, Cp, w_tiled, wt_tiled)
                self.prep_table.append((self.device_table(arr), len(ent), dt))
        if self.prep_h2 and (self.prep_h2_table is None or self.prep_h2_table[1] != len(self.prep_h2)):
            # fp16 planes of every weight copy (f16x2): one table, two launches
            arr = (_lib.H2Desc * len(self.prep_h2))()
            for i, (x, rows, Cc, ld, planes, pstride, ldp, layout, work, _) in enumerate(self.prep_h2):
                arr[i] = _lib.H2Desc(x, planes, work, rows, pstride, Cc, ld, ldp, layout)
            self.prep_h2_table = (self.device_table(arr), len(self.prep_h2))
        cut = self.prep_cut if (overlap and self.training and self.sw.prep_overlap and len(self.prep_table) == 1) else None
        if cut is not None and 0 < cut[1] < self.prep_table[0][1] and self.prep_h2 and 0 < cut[2] < len(self.prep_h2):
            # early part on the caller's stream, the rest on the side stream (which first picks up the caller's stream: the masters)
            tab, n, dt = self.prep_table[0]
            nA, hA = cut[1], cut[2]
            main, side = torch.cuda.current_stream(self.device), self.e.side_stream(self.device)
            side.wait_stream(main)
            ss = side.cuda_stream
            _lib.check(self.lib.dml_prep_weights(tab.data_ptr(), nA, dt, stream), "dml_prep_weights")
            _lib.check(self.lib.dml_h2_split_table(self.prep_h2_table[0].data_ptr(), hA, stream), "dml_h2_split_table")
            _lib.check(self.lib.dml_prep_weights(tab.data_ptr() + nA * C.sizeof(_lib.PrepDesc), n - nA, dt, ss), "dml_prep_weights")
            for g in self.prep_gather:
                _lib.check(self.lib.dml_gather_taps(*g, ss), "dml_gather_taps")
            _lib.check(self.lib.dml_h2_split_table(self.prep_h2_table[0].data_ptr() + hA * C.sizeof(_lib.H2Desc),
                                                   len(self.prep_h2) - hA, ss), "dml_h2_split_table")
            if getattr(self, "_prep_ev", None) is None:
                self._prep_ev = torch.cuda.Event()
            self._prep_ev.record(side)
            self.prep_event = self._prep_ev
        else:
            for tab, n, dt in self.prep_table:
                _lib.check(self.lib.dml_prep_weights(tab.data_ptr(), n, dt, stream), "dml_prep_weights")
            for g in self.prep_gather:
                _lib.check(self.lib.dml_gather_taps(*g, stream), "dml_gather_taps")
            if self.prep_h2:
                _lib.check(self.lib.dml_h2_split_table(self.prep_h2_table[0].data_ptr(), self.prep_h2_table[1], stream),
                           "dml_h2_split_table")
        self.prepped_version = key

    # ---- replay: one C call per contiguous run of ops (dml_plan_run) unless the engine is told to stay in Python
    def _native_list(self, ops):
        key = id(ops)
        nat = self._nat.get(key)
        if nat is None:
            nat = NativeList(self.lib, ops, self.side if ops is self.bwd else None)
            # an aborted replay may leave tickets of a K-split tail (DmlConvDesc.tail_counters) behind: the counters must be
            # zero when the next launch that uses them starts
            nat.on_error = self.tail_cnt.zero_
            self._nat[key] = nat
        return nat

    def _events(self):
        if self._ev_handles is None:
            cur = torch.cuda.current_stream(self.device)
            self._ev_objs = [torch.cuda.Event() for _ in range(16)]
            for e in self._ev_objs:
                e.record(cur)                       # instantiates the hipEvent_t
            self._ev_handles = (C.c_void_p * len(self._ev_objs))(*[e.cuda_event for e in self._ev_objs])
        return self._ev_handles

    def _mark_events(self, n):
        """n (main, side) event pairs for the deferred hooks of _exec, instantiated once"""
        evs = getattr(self, "_mark_ev", [])
        cur = torch.cuda.current_stream(self.device)
        while len(evs) < n:
            pair = (torch.cuda.Event(), torch.cuda.Event())
            for e in pair:
                e.record(cur)                       # instantiates the hipEvent_t
            evs.append(pair)
        self._mark_ev = evs
        return evs[:n]

    # ---- ops[start:stop] in order: Plan._exec (dmlnet/engine.py) chooses between these two
    def _exec_python(self, run, ops, stream, start, stop, hook, skip_ranges, side_stream):
        """op by op from Python (DML_NATIVE_PLAN=0, profiling); run: the replay loop, Plan.run or what bench.py put in its place"""
        skipped = set()
        for (lo, hi) in skip_ranges:
            skipped.update(range(lo, hi))
        if side_stream is not None:
            return self._py_backward_two_streams(ops, stream, side_stream, hook, skipped)
        return run(ops, stream, start, stop, hook=hook, skipped=skipped)

    def _exec_native(self, ops, stream, start, stop, hook, skip_ranges, side_stream):
        """Native segments run through dml_plan_run; Python steps (collectives), skipped ranges and the hook points (hook.points: op
        indices after which hook(i) must run -- the gradient buckets of the data-parallel reducer) cut the list into segments."""
        nat = self._native_list(ops)
        points = getattr(hook, "points", None) if hook is not None else ()
        if hook is not None and points is None:
            points = range(start, stop)              # a hook without declared points wants every op
        # A DEFERRED hook (hook.deferred: the data-parallel reducer) only enqueues work on another stream that has to wait for this
        # point of the list: the native replay records an event pair (main / side stream) after each of its ops (dml_plan_run_marks)
        # and the hook runs once the whole list has been enqueued, hook(op, main event, side event) -- one return to Python per
        # backward instead of one per gradient bucket.
        deferred = hook is not None and getattr(hook, "deferred", False) and points is not None
        marks, mark_ops, mark_evs = None, [], []
        if deferred:
            mark_ops = sorted(k for k in points if start <= k < stop)
            mark_evs = self._mark_events(len(mark_ops))
            if mark_ops:
                arr = (C.c_int32 * len(mark_ops))(*mark_ops)
                hnd = (C.c_void_p * (2 * len(mark_ops)))(*[e.cuda_event for pair in mark_evs for e in pair])
                marks = (arr, len(mark_ops), hnd)
                self.keep_marks = (arr, hnd)
            points = ()
        cuts = set(nat.python_ops)
        cuts.update(points)
        skips = sorted((max(lo, start), min(hi, stop)) for (lo, hi) in skip_ranges if lo < stop and hi > start)
        events = self._events() if side_stream is not None else None
        n_ev = len(events) if events is not None else 0
        i = start
        order = sorted(c for c in cuts if start <= c < stop)
        ci, si = 0, 0
        while i < stop:
            while si < len(skips) and skips[si][1] <= i:
                si += 1
            if si < len(skips) and skips[si][0] <= i:      # inside a skipped range: only the hook points fire
                hi = skips[si][1]
                for k, (em, es) in zip(mark_ops, mark_evs):      # (deferred hooks: their events, recorded here)
                    if i <= k < hi:
                        em.record(torch.cuda.current_stream(self.device))
                        if side_stream is not None:
                            es.record(self.e.side_stream(self.device))
                if hook is not None:
                    for k in order:
                        if i <= k < hi and k in points:
                            hook(k)
                i = hi
                continue
            end = skips[si][0] if si < len(skips) else stop
            while ci < len(order) and order[ci] < i:
                ci += 1
            if ci < len(order) and order[ci] < end:
                k = order[ci]
                if k in nat.python_ops:
                    if k > i:
                        nat.run(i, k, stream, side_stream, events, n_ev, marks)
                    fn, args = ops[k]
                    fn(*args, stream)
                    if k in mark_ops:                # (a Python step that is a mark itself)
                        em, es = mark_evs[mark_ops.index(k)]
                        em.record(torch.cuda.current_stream(self.device))
                        if side_stream is not None:
                            es.record(self.e.side_stream(self.device))
                else:
                    nat.run(i, k + 1, stream, side_stream, events, n_ev, marks)
                if hook is not None and k in points:
                    hook(k)
                i = k + 1
            else:
                nat.run(i, end, stream, side_stream, events, n_ev, marks)
                i = end
        for k, (em, es) in zip(mark_ops, mark_evs):
            hook(k, em, es if side_stream is not None else None)

    def run_backward(self, hook=None):
        """Replay the backward plan: weight gradients on the engine's side stream, everything else on the
        caller's current stream; joined at the end."""
        main = torch.cuda.current_stream(self.device)
        skip = tuple(getattr(self, "skip_ranges", ()))
        if not self.e.overlap_wgrad or not self.side:
            self._exec(self.bwd, main.cuda_stream, hook=hook, skip_ranges=skip)
            return
        side = self.e.side_stream(self.device)
        side.wait_stream(main)
        self._exec(self.bwd, main.cuda_stream, hook=hook, skip_ranges=skip, side_stream=side.cuda_stream)
        main.wait_stream(side)

    def _py_backward_two_streams(self, ops, ms, ss, hook, skipped):
        """the Python replay of the two-stream backward (DML_NATIVE_PLAN=0, profiling)"""
        main = torch.cuda.current_stream(self.device)
        side = self.e.side_stream(self.device)
        if self._side_events is None:
            self._side_events = {i: torch.cuda.Event() for i, f in self.side.items() if f}
        sidemap, events = self.side, self._side_events
        for i, (fn, args) in enumerate(ops):
            if i in skipped:
                if hook is not None:
                    hook(i)
                continue
            flag = sidemap.get(i)
            if flag is None:
                rc = fn(*args, ms)
            else:
                if flag:
                    ev = events[i]
                    ev.record(main)
                    side.wait_event(ev)
                rc = fn(*args, ss)
            if rc:
                _lib.check(rc, getattr(fn, "__name__", "kernel") + " (bwd op %d)" % i)
            if hook is not None:
                hook(i)

    def run_forward(self, stream):
        """Replay the forward plan.  Inference plans carry fork groups (`fwd_forks`: the independent ASPP branches): their
        op ranges run side by side on the engine's branch streams and join on the caller's stream -- at batch 1 each
        branch is a grid of 128-256 workgroups, too small to fill the chip alone."""
        forks = getattr(self, "fwd_forks", None)
        if not forks:
            ev = getattr(self, "prep_event", None)
            if ev is not None and self.prep_cut is not None:
                # (refresh_weights, overlap: the weight copies of layer2.. are being made on the side stream)
                self._exec(self.fwd, stream, 0, self.prep_cut[0])
                torch.cuda.current_stream(self.device).wait_event(ev)
                self.prep_event = None
                self._exec(self.fwd, stream, self.prep_cut[0], len(self.fwd))
                return
            self._exec(self.fwd, stream)
            return
        main = torch.cuda.current_stream(self.device)
        pos = 0
        for ranges in forks:
            self._exec(self.fwd, stream, pos, ranges[0][0])
            streams = self.e.branch_streams(self.device, len(ranges))
            for (lo, hi), s in zip(ranges, streams):
                s.wait_stream(main)
                self._exec(self.fwd, s.cuda_stream, lo, hi)
            for s in streams[:len(ranges)]:
                main.wait_stream(s)
            pos = ranges[-1][1]
        self._exec(self.fwd, stream, pos, len(self.fwd))

    @staticmethod
    def run(ops, stream, start=0, stop=None, hook=None, skipped=()):
        stop = len(ops) if stop is None else stop
        for i in range(start, stop):
            if i in skipped:
                if hook is not None:
                    hook(i)
                continue
            fn, args = ops[i]
            rc = fn(*args, stream)
            if rc:
                _lib.check(rc, getattr(fn, "__name__", "kernel") + " (op %d)" % i)
            if hook is not None:
                hook(i)

    _py_run = run          # bench.py's profiled pass replaces Plan.run: the native path then steps aside
