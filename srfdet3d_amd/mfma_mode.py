"""What the opt-in "bf16 products on f32 tensors" modes share: `nhwc.mfma_dtype` (image branch, inference), `sparse.mfma_dtype` (sparse
encoder, inference) and `train_conv.mfma_dtype` (camera branch under autograd) are subclasses of `MfmaMode` that add a name and the
documentation of their mode.  The rules live here, once: off by default, `mfma_dtype(None)` switches an outer context of the same mode
off, a refusal is reported with its reason, a mode that was asked for and launched nothing is an error.  The modes are independent:
each subclass has its own innermost context.  Process-wide while open (the executors are single-threaded); not an environment variable.

The next mode is a subclass with its docstring, a `*_bf16_why_not` next to its kernels' other limits in `ops` (None, or the reason a
layer keeps its f32 route), and a property line on the detector (`SRFDet._mfma_arg`)."""
import torch


class MfmaMode:
    def __init_subclass__(cls, **kw):
        super().__init_subclass__(**kw)
        cls._innermost = None          # the innermost open context of this mode, or None: every layer on its f32 route

    def __init__(self, dtype, routes=None):
        """routes: a list that receives one record per executed layer (and direction); `launches` counts those on the bf16 kernels."""
        if dtype is not None and dtype != torch.bfloat16:
            name = f"{type(self).__module__.rpartition('.')[2]}.{type(self).__name__}"
            raise ValueError(f"{name}: only torch.bfloat16 (or None) is implemented, not {dtype}")
        self.dtype, self.routes, self.launches = dtype, routes, 0

    def __enter__(self):
        cls = type(self)
        self._outer, cls._innermost = cls._innermost, (self if self.dtype is not None else None)
        return self

    def __exit__(self, *exc):
        type(self)._innermost = self._outer
        return False

    @classmethod
    def active(cls):
        """The innermost open context of this mode, or None (none is open, or `mfma_dtype(None)` hides it)."""
        return cls._innermost

    def report(self, layer, why, **extra):
        """One executed layer (extra: direction=): `why` is the reason it keeps its f32 route, falsy when it runs on the bf16 kernels.
        -> whether it does."""
        if self.routes is not None:
            self.routes.append(dict(layer=layer, **extra, route="f32" if why else "bf16", why=why))
        self.launches += not why
        return not why

    def require_launches(self, message):
        """After a pass: a mode that was asked for and took no layer is an error, never a quiet f32 pass."""
        if self.dtype is not None and self.launches == 0:
            raise RuntimeError(message)
