"""The LCLD classifier (mirror of src/experiments/lcld/model.py:9-42): Dense 64-32-16 relu,
Dense 2 softmax, trained on the device (moeva2_amd/experiments/training.py)."""
from .. import training

HIDDEN = (64, 32, 16, 2)


def create_model(n_features, seed=42):
    """A freshly initialised model (Glorot-uniform kernels, zero biases)."""
    return training.glorot_model((int(n_features),) + HIDDEN, seed)


def train_model(x_train_s, y_train, seed=42, epochs=100, batch_size=512, patience=25,
                return_info=False, trainer_factory=training.DeviceTrainer):
    """model.py:23-42 on scaled rows; y as class indices or one-hot rows."""
    model = create_model(x_train_s.shape[1], seed)
    return training.fit(model, x_train_s, y_train, seed=seed, epochs=epochs,
                        batch_size=batch_size, patience=patience, return_info=return_info,
                        trainer_factory=trainer_factory)
