from openvoice_amd.mel_processing import (  # noqa: F401
    dynamic_range_compression_torch, dynamic_range_decompression_torch, mel_spectrogram_torch, spec_to_mel_torch,
    spectral_de_normalize_torch, spectral_normalize_torch, spectrogram_torch)
