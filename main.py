"""Entry point with the reference's shape (main.py:12-55): ``main(load_config())`` dispatches on
``config.task`` / ``config.function``.  The inference path, scoring against label files, fine-tuning ("adapt") and training a PyanNet2
or a PyanNet from initialisation ("train") are in scope; every other task of the reference (corpus download / preparation) raises with a pointer to
SURVEY.md."""
import faulthandler

faulthandler.enable()

from config.config import load_config  # noqa: E402
from src.scripts import adapt_vad, predict_vad, test_vad, train_vad    # noqa: E402


def main(config):
    if config.task == "run":
        if config.function == "predict":
            return predict_vad(**config)
        if config.function == "test":
            return test_vad(**config)
        if config.function == "adapt":
            return adapt_vad(**config)
        if config.function == "train":
            return train_vad(**config)
        raise NotImplementedError(f"function={config.function!r}: only 'predict', 'test', 'adapt' and 'train' are on the accelerated path")
    raise NotImplementedError(f"task={config.task!r}: data preparation tasks are out of scope (SURVEY.md section 2)")


if __name__ == "__main__":
    import torch

    print("GPU:", torch.cuda.is_available())
    main(load_config())
