from .packed_rf_tracer import PackedRFTracer
from .packed_sdf_tracer import PackedSDFTracer
from .packed_spc_tracer import PackedSPCTracer

__all__ = ["PackedRFTracer", "PackedSDFTracer", "PackedSPCTracer"]
