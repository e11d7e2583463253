from .stream_metrics import StreamSegMetrics, AverageMeter  # noqa: F401
from .open_set import OpenSetSweepMetrics  # noqa: F401
