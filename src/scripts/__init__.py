from uvad_amd.scripts import adapt_vad, predict_vad, test_vad, train_vad  # noqa: F401

__all__ = ["adapt_vad", "predict_vad", "test_vad", "train_vad"]
