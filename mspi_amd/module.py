"""Base class of every HIP-backed nn.Module: torch layers are kept only as named parameter
holders (so state-dict keys equal the reference's), the arithmetic runs from a packed plan
that is rebuilt whenever the parameters may have changed.

When plans are rebuilt ("When plans are rebuilt"): a plan is keyed by the
(data_ptr, _version) of every parameter and buffer of its owner's SUBTREE -- a superset of what
any `_pack` reads, children's tensors and BatchNorm statistics included.  `pk` compares before it
hands the plan out, so a load_state_dict / .to() / optimiser step / in-place write anywhere below
the owner, through a HipModule or through a plain nn container, drops the plan.  Calling a
HipModule validates its whole subtree ONCE for the duration of the call (two list comparisons
over the subtree's tensors); the `pk` accesses of the nested run() methods are a set look-up."""
import contextlib
import threading

import torch
import torch.nn as nn
from torch.nn.modules import module as _nn_module

from ._lib import MspiError

_scope = threading.local()        # .valid: ids of the HipModules validated for the call that runs in this thread, or None
_STRUCT = [0]                     # bumped whenever ANY module registers a parameter, a buffer or a child: flat lists are stale
_data_ptr = torch.Tensor.data_ptr


def _bump(*_):
    _STRUCT[0] += 1


_nn_module.register_module_parameter_registration_hook(_bump)
_nn_module.register_module_buffer_registration_hook(_bump)
_nn_module.register_module_module_registration_hook(_bump)


def _flatten(m, out, full):
    """The parameters and buffers below m in registration order.  full=False leaves out what no plan key holds: children
    that are keyed on their own (_PK_SELF_KEYED) and BatchNorm's step counter, which nothing packs."""
    out.extend(t for t in m._parameters.values() if t is not None)
    out.extend(t for n, t in m._buffers.items() if t is not None and (full or n != "num_batches_tracked"))
    skip = () if full or not isinstance(m, HipModule) else m._PK_SELF_KEYED
    for n, c in m._modules.items():
        if c is not None and n not in skip:
            _flatten(c, out, full)
    return out


class TensorWatch:
    """The parameters and buffers below some modules as they are now: same() is True while none of them has been loaded
    into, moved, stepped, written in place or replaced by another tensor.
    _version is torch's private in-place counter, the only record of optimiser steps and of load_state_dict (both write in
    place and keep data_ptr); `p.data = ...` (nn.Module._apply) need not bump it but moves data_ptr.  The watch holds the
    storages it names, so storage that replaces them (.double().float(), .to(copy=True)) cannot come back at an old address.
    The tensor list is walked again only after some module of the process registered a parameter, a buffer or a child.
    Not seen: a Parameter object swapped for another by a direct write to a plain container's `_parameters` dict
    (torch.__future__.set_overwrite_module_params_on_conversion), and tensors that are neither parameters nor buffers."""
    __slots__ = ("roots", "full", "struct", "ts", "vers", "ptrs", "hold", "ids")

    def __init__(self, roots, ids=(), full=True):
        self.roots, self.full, self.struct, self.ids = tuple(roots), full, _STRUCT[0], ids
        self.ts = ts = [t for r in self.roots for t in _flatten(r, [], full)]
        self.vers = [t._version for t in ts]
        self.ptrs = list(map(_data_ptr, ts))
        self.hold = [t.untyped_storage() for t in ts]

    def same(self):
        ts = self.ts
        if self.struct != _STRUCT[0]:
            struct = _STRUCT[0]
            now = [t for r in self.roots for t in _flatten(r, [], self.full)]
            if len(now) != len(ts) or any(a is not b for a, b in zip(now, ts)):
                return False
            self.struct = struct
        return [t._version for t in ts] == self.vers and list(map(_data_ptr, ts)) == self.ptrs


def _flatten_own(m):
    return [t for t in m._parameters.values() if t is not None] + \
        [t for n, t in m._buffers.items() if t is not None and n != "num_batches_tracked"]


def _scan(m, ids):
    """Nested tuple of (data_ptr, _version) over what _flatten(m, full=False) walks; every HipModule in it compares its own
    subtree's key with the one its plan was built under and drops a stale plan.  Appends the HipModules' ids."""
    key = [(t.data_ptr(), t._version) for t in _flatten_own(m)]
    hip = isinstance(m, HipModule)
    skip = m._PK_SELF_KEYED if hip else ()
    for name, c in m._modules.items():
        if c is not None and name not in skip:
            key.append(_scan(c, ids))
    key = tuple(key)
    if hip:
        ids.append(id(m))
        m._validate(key)
    return key


def _check(m):
    """Validate the plans of m's subtree against the tensors' present state; returns the ids of its HipModules."""
    d = m.__dict__
    w = d.get("_pk_watch")
    if w is not None and w.same():
        if m._PK_SELF_KEYED and d.get("_pk") is not None:
            m._pk_refresh(d["_pk"])
        return w.ids
    w = TensorWatch((m,), full=False)        # taken BEFORE the plans are compared: whatever moves later fails this watch
    ids = []
    _scan(m, ids)
    w.ids = frozenset(ids)
    d["_pk_watch"] = w
    return w.ids


class HipModule(nn.Module):
    _PK_SELF_KEYED = ()      # direct children whose packs carry keys of their own inside the plan (see _pk_refresh)

    def _invalidate(self):
        _bump()
        for m in self.modules():
            d = m.__dict__
            d.pop("_pk", None)
            d.pop("_pk_key", None)
            d.pop("_pk_watch", None)

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        self._invalidate()
        return r

    def load_state_dict(self, *a, **k):
        r = super().load_state_dict(*a, **k)
        self._invalidate()
        return r

    def _pack(self):
        raise NotImplementedError

    def _pk_refresh(self, pk):
        """Bring the parts of a still-valid plan that follow keys of their own (_PK_SELF_KEYED) up to date."""

    def _validate(self, key):
        d = self.__dict__
        if d.get("_pk_key") != key:
            d.pop("_pk", None)
            d["_pk_key"] = key
        elif self._PK_SELF_KEYED and d.get("_pk") is not None:
            self._pk_refresh(d["_pk"])

    @property
    def pk(self):
        """Packed weights (BN folded, channel-minor taps), built lazily on the parameters' device from the parameters'
        present values: outside a validated call every access compares the subtree's tensors with their recorded state."""
        d = self.__dict__
        valid = getattr(_scope, "valid", None)
        if valid is None or id(self) not in valid:
            _check(self)
        if "_pk" not in d:
            with torch.no_grad():
                d["_pk"] = self._pack()
        return d["_pk"]

    @contextlib.contextmanager
    def plans_checked(self):
        """One validation of this module's subtree for everything that runs inside (an entry point that is not __call__)."""
        valid = getattr(_scope, "valid", None)
        if valid is not None:
            if id(self) not in valid:
                _check(self)
            yield
            return
        _scope.valid = _check(self)
        try:
            yield
        finally:
            _scope.valid = None

    def __call__(self, *a, **k):
        valid = getattr(_scope, "valid", None)
        if valid is not None:
            if id(self) not in valid:
                _check(self)
            return super().__call__(*a, **k)
        _scope.valid = _check(self)
        try:
            return super().__call__(*a, **k)
        finally:
            _scope.valid = None

    def _check_eval(self):
        if self.training:
            raise MspiError("%s is an inference engine (BatchNorm is folded into the convolutions): call .eval()"
                            % type(self).__name__)


def to_cl(x):
    """Accept a CL or an NCDHW tensor (e.g. from a user-supplied backbone) as a head input."""
    from .engine import CL, rup4
    if isinstance(x, CL):
        return x
    N, Cc, T, H, W = x.shape
    if x.stride(1) == 1 and x.stride(4) % 4 == 0 and x.stride(3) == W * x.stride(4) and x.stride(2) == H * x.stride(3):
        return CL(x, 0, N, T, H, W, Cc, x.stride(4), x.stride(0))
    ld = rup4(Cc)
    buf = torch.zeros(N, T, H, W, ld, dtype=torch.float32, device=x.device)
    buf[..., :Cc] = x.permute(0, 2, 3, 4, 1)
    return CL(buf.view(-1), 0, N, T, H, W, Cc, ld)
