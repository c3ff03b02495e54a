"""se_snmf_nat_amd -- MI355X-native sparse-NMF multiplicative-update engine.

Drop-in for the hot path of lordet01/SE_SNMF_NAT (src/sparse_nmf.m, src/sparse_nmf_GPU.m and
the basis-training loop of run_basis_DNMF.m) behind the same function signature.  The compute
lives in libsnmf_hip.so (hand-written HIP for gfx950, C ABI in include/snmf.h); this package is
the host-side mirror of the reference interface.  There is no CPU fallback.
"""
from .api import (Context, Plan, SnmfError, default_context, dnmf_adapt, run_basis_dnmf, snmf_mdi, snmf_mdi_Sm,  # noqa: F401
                  sparse_nmf, sparse_nmf_GPU)
from .batch import (BatchPlan, BatchPlan64, BatchPlanMdi64, run_basis_dnmf_batch, snmf_mdi_batch, snmf_mdi_Sm_batch,  # noqa: F401
                    sparse_nmf_batch, sparse_nmf_batch_fp64)
from .frontend import stft_features_batch  # noqa: F401
from .train import (TrainSignals, assemble_training_signals, run_basis_DNMF_batch, run_basis_DNMF_Mel_batch,  # noqa: F401
                    run_basis_train_assembled_batch, run_basis_train_clips_batch, run_basis_train_signal_batch)


def release_device_lists():
    """Give back what the multi-device entries keep per device list for the life of the process (contexts, pinned bounce
    buffers, gather buffers: snmf_multi_release_cache in include/snmf.h).  Returns the number of idle teams destroyed."""
    from . import _lib
    return int(_lib.load().snmf_multi_release_cache())


__version__ = "0.1.0"
