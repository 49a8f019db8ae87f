"""phantomsdr_amd — MI355X-native spectrum-distributor DSP core.

One hot path of PhantomSDR, re-built as hand-written HIP for gfx950 behind a C-ABI
(include/psdr.h): windowed 50 %-overlap forward FFT -> per-client slice + small inverse
DFT demodulation -> waterfall power pyramid + int8 quantisation.  See DESIGN.md.

Importing this package requires the built HIP library (phantomsdr_amd/libpsdr_hip.so);
there is no CPU implementation behind it.
"""
from ._lib import PsdrError, load  # noqa: F401
from .core import AF_DEEMPHASIS, AF_HIGHPASS, AF_KINDS, AF_LOWPASS, AF_PEAK, AUDIO_FILTER_SECTIONS, design_audio_filter  # noqa: F401
from .core import NR_LIGHT, NR_NORMAL, NR_PRESETS, NR_STRONG, noise_reduction_preset  # noqa: F401
from .core import ANB_LIGHT, ANB_NORMAL, ANB_PRESETS, ANB_STRONG, audio_blanker_preset  # noqa: F401
from .core import SCAN_MAX_SIGNALS, SIGNAL_DTYPE  # noqa: F401
from .core import TONE_ANY, tone_defaults, tone_table  # noqa: F401
from .core import cw_defaults  # noqa: F401
from .core import rtty_defaults  # noqa: F401
from .core import psk_defaults  # noqa: F401
from .core import FAX_AUTO, FAX_FREE, fax_defaults  # noqa: F401
from .core import AGC_FAST, AGC_PRESETS, AGC_REFERENCE, AGC_SLOW, agc_preset  # noqa: F401
from .core import (AM, FM, IQ, LSB, MODES, SAM, SAM_BOTH, SAM_LOWER, SAM_SIDEBANDS, SAM_UPPER, USB, WF_DETECTORS, WF_MEAN, WF_PEAK,  # noqa: F401
                   WF_SAMPLE, AudioClient, Context, Group, HipFFT, SpectrumEngine, WaterfallClient, derived_params)

load()  # fail loudly at import time if the extension is missing
