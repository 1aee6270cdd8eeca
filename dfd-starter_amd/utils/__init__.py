from .adaptive_omega import AdaptiveOmega  # noqa: F401
from .noise_sources import CounterNoiseSource, SharedNoiseTable, SimpleNoiseSource, RNGNoiseSource  # noqa: F401
