"""Native launch lists (dml_plan_run): the packed copy of a plan's op list that one C call replays."""
# The argument lists of the ops write through to it when a per-step pointer, seed or momentum is patched.
import ctypes as C
import struct

from . import _lib

_M64 = 0xFFFFFFFFFFFFFFFF


def _pack_word(v, ctype):
    """one argument -> (64-bit word, indirect flag) in the convention of DmlPlanOp (include/dmlnet_hip.h)"""
    if v is None:
        return 0, False
    if ctype is C.c_float:
        return struct.unpack("<I", struct.pack("<f", float(v)))[0], False
    if ctype is C.c_double:
        return struct.unpack("<Q", struct.pack("<d", float(v)))[0], False
    if isinstance(v, int):
        return v & _M64, False
    if hasattr(v, "_obj"):                         # C.byref(x): the address of x (descriptor structs, int* out-parameters)
        return C.addressof(v._obj), False
    if isinstance(v, C._SimpleCData):              # a c_int passed by value that another op fills in at issue time
        if C.sizeof(v) != 4:
            raise TypeError("only 32-bit indirect arguments are supported")
        return C.addressof(v), True
    raise TypeError("cannot pack plan argument %r for %r" % (v, ctype))


class BoundArgs(list):
    """The argument list of one plan op.  Plain list for the Python replay; once the op has a slot in a native launch
    list, item assignment (per-step pointers, seeds, momenta) writes through to the packed copy."""
    __slots__ = ("slot", "types", "meta")

    def __init__(self, it=()):
        super().__init__(it)
        self.slot, self.types, self.meta = None, None, None

    def __setitem__(self, k, v):
        super().__setitem__(k, v)
        if self.slot is not None:
            w, ind = _pack_word(v, self.types[k])
            self.slot.args[k] = w
            if ind:
                self.slot.indirect |= (1 << k)
            else:
                self.slot.indirect &= ~(1 << k) & 0xFFFFFFFF


class NativeList:
    """Packed copy of a plan's op list for dml_plan_run; ops that are Python callables (collectives) stay outside."""

    def __init__(self, lib, ops, side=None):
        self.lib = lib
        n = len(ops)
        self.arr = (_lib.PlanOp * max(n, 1))()
        self.python_ops = set()
        ids = {}
        for i, (fn, args) in enumerate(ops):
            name = getattr(fn, "__name__", None)
            types = getattr(fn, "argtypes", None)
            if name is None or types is None or not name.startswith("dml_"):
                self.python_ops.add(i)
                self.arr[i].fn = -1
                continue
            if name not in ids:
                ids[name] = lib.dml_plan_fn_id(name.encode())
            fid = ids[name]
            if fid < 0 or lib.dml_plan_fn_nargs(fid) != len(args) or len(args) > _lib.PLAN_MAX_ARGS \
                    or len(types) != len(args) + 1:
                raise RuntimeError("plan op %d (%s) does not fit the native launch list" % (i, name))
            slot = self.arr[i]
            slot.fn, slot.nargs, slot.indirect = fid, len(args), 0
            flag = side.get(i) if side else None
            slot.stream, slot.wait = (0, 0) if flag is None else (1, 1 if flag else 0)
            if not isinstance(args, BoundArgs):
                raise TypeError("plan op arguments must come from Plan.call()")
            args.slot, args.types = slot, types
            for k, v in enumerate(args):
                args[k] = v                          # packs through __setitem__
        self.n = n
        self.failed = C.c_int(-1)
        self.on_error = None

    def run(self, first, last, stream, side_stream=None, events=None, n_events=0, marks=None):
        if marks is not None:      # (marks, count, event handles): dml_plan_run_marks records an event pair after each marked op
            rc = self.lib.dml_plan_run_marks(self.arr, first, last, stream, side_stream, events, n_events, marks[0], marks[1], marks[2],
                                             C.byref(self.failed))
        else:
            rc = self.lib.dml_plan_run(self.arr, first, last, stream, side_stream, events, n_events, C.byref(self.failed))
        if rc:
            if self.on_error is not None:
                self.on_error()
            _lib.check(rc, "native plan op %d" % self.failed.value)
