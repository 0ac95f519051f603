"""Drop-in for the feature functions of ``SpeakerIdentification/scripts/speaker_identification.py``.

``input_feature_gen`` (:372-398) and ``delta`` (:141-151) keep their names and return values;
the MFCC / delta / delta-delta / pad-to-256 path runs in the ``si_fe`` HIP kernel (float64 math).
``make_feature_experiment`` (:317-369), used by the registration/transfer-learning callers, keeps
its chunked output layout.  ``transfer_learning`` (:401-477) and ``transfer_learning_on_experiment``
(:480-503), the speaker registration of ``record_on_pc.py:340-346``, run the frozen base once
(``si_embed``) and fit the sigmoid head in one persistent kernel (``si_train.hip``), optionally
fine-tune the whole network (stage 2, ``fine_tune=True``: ``si_bwd.hip``), then write the deployed
model with ``tfbundle.save_deployed``.
"""
import math
import os
import sys
import time
from collections import namedtuple

import numpy as np
import scipy.io.wavfile as _wavfile

from . import _lib


def delta(feat, N):
    """speaker_identification.py:141-151 (edge-padded regression delta), vectorised on the host.
    Exposed for API compatibility; the batched GPU path computes deltas inside the kernel."""
    feat = np.asarray(feat)
    denominator = 2 * sum([i ** 2 for i in range(1, N + 1)])
    padded = np.pad(feat, ((N, N), (0, 0)), mode='edge')
    t = len(feat)
    out = np.zeros_like(feat, dtype=np.result_type(feat.dtype, np.float64))
    for n in range(-N, N + 1):
        if n:
            out = out + n * padded[N + n:N + n + t]
    return (out / denominator).astype(np.result_type(feat.dtype, np.float64))


def _read(path):
    rate, sig = _wavfile.read(path)
    if rate != 16000:
        raise ValueError(f'{path}: the HIP MFCC is built for 16 kHz, got {rate}')
    if sig.dtype != np.int16 or sig.ndim != 1:
        raise ValueError(f'{path}: expected mono int16 PCM')
    return sig


def input_feature_gen(wav_path, device=None):
    """-> 'silent' (fewer than 4000 samples) or float64 [1, 256, 39] (:372-398)."""
    sig = _read(wav_path)
    if len(sig) < _lib.SI_SILENT_LEN:
        return 'silent'
    feat, silent = _lib.default_context(device).si_features(sig[None], lens=np.array([len(sig)], np.int32))
    return feat.astype(np.float64)


def input_feature_batch(pcm, lens=None, device=None):
    """Batched input_feature_gen: int16 [n, L] (or list) -> (float32 [n, 256, 39], silent [n])."""
    return _lib.default_context(device).si_features(pcm, lens=lens)


_speakers_count_dict = {}   # the reference binarizer's mutable default argument: process-wide


def binarizer(str_list, dim, speakers_count_dict=_speakers_count_dict):
    """speaker_identification.py:122-138, same semantics: first-occurrence numbering that restarts
    at 0 on every call while the dict (a mutable default argument) keeps the labels of earlier
    calls -- so a new speaker in a later call can share an index with an old one, and an index
    >= dim raises IndexError, exactly as in the reference."""
    if not str_list:
        raise UnboundLocalError("local variable 'result' referenced before assignment")
    count = 0
    rows = np.zeros((len(str_list), dim))
    for i, s in enumerate(str_list):
        if s not in speakers_count_dict:
            speakers_count_dict[s] = count
            count += 1
        rows[i, speakers_count_dict[s]] = 1
    return rows


def make_feature_experiment(wav_files, device=None):
    """(:317-369): per file MFCC+deltas over the WHOLE file, zero-padded to a multiple of 256 frames
    and cut into 256-frame windows; labels = file stem; returns (x float64 [S,256,39], one-hot y,
    speaker_id dict) with the reference's binarizer (state kept across calls).  Whole-file features
    are produced chunk-aligned on the GPU (see conversation_features)."""
    train_x, train_y = [], []
    begin = time.time()
    for i, onewav in enumerate(wav_files):
        if i % 5 == 4:
            gap = time.time() - begin
            sys.stdout.write('\r%.2f %% used:%ds' % (float(i) * 100 / len(wav_files), gap))
        label = os.path.basename(onewav)[:-4]
        chunks = conversation_features(_read(onewav), device=device)
        for c in chunks:
            train_x.append(c)
            train_y.append(label)
    y = binarizer(train_y, dim=len(set(train_y)))
    speaker_id = {str(int(np.argmax(y[i]))): train_y[i] for i in range(len(train_y))}
    return np.asarray(train_x), y, speaker_id


def get_wav_files(wav_path):
    """speaker_identification.py:57-66: every .wav / .WAV under wav_path of at least 240000 bytes
    (7.5 s); sorted here, where the reference keeps os.walk's order, so that the speaker numbering
    does not depend on the file system."""
    wav_files = []
    for dirpath, _, filenames in os.walk(wav_path):
        for filename in filenames:
            if filename.endswith('.wav') or filename.endswith('.WAV'):
                path = os.sep.join([dirpath, filename])
                if os.stat(path).st_size >= 240000:
                    wav_files.append(path)
    return sorted(wav_files)


def _stratified_split(rng, idx, labels, ratio):
    """-> (keep, held_out) index arrays: per class round(ratio * n_c) samples held out, but at least
    one on each side for every class with two or more samples (a class of one stays in `keep`)"""
    keep, out = [], []
    for c in np.unique(labels[idx]):
        members = idx[labels[idx] == c]
        members = members[rng.permutation(len(members))]
        n_out = 0
        if len(members) >= 2:
            n_out = min(max(int(round(ratio * len(members))), 1), len(members) - 1)
        out.append(members[:n_out])
        keep.append(members[n_out:])
    return np.sort(np.concatenate(keep)), np.sort(np.concatenate(out))


def _fit_plan(labels, K, seed, test_split_ratio, epochs, restarts, fine_tune_epochs=0):
    """Everything random about one registration, drawn with numpy from `seed`: the stratified test
    split (only when test_split_ratio > 0) and 70/30 validation split, and per restart the
    Glorot-uniform initial head (limit sqrt(6 / (512 + K)), zero bias) and the sample order of every
    epoch.  Restart r's draws come from their own generator, so they do not depend on `restarts`.
    Neither sklearn's train_test_split nor TensorFlow's initialiser and shuffle streams are reproduced:
    the same seed gives a different (equally distributed) split, head and order than the reference.
    fine_tune_epochs > 0 adds perm2, the sample order of every stage-2 epoch, from a generator of its
    own: every other entry of the plan is the one a stage-1-only registration draws.
    -> dict(train, val, test index arrays; w0 [R,512,K] f32; b0 [R,K] f32; perm [R,epochs,n_train] i32;
    perm2 [fine_tune_epochs,n_train] i32)"""
    labels = np.asarray(labels)
    rng = np.random.default_rng([int(seed), 0])
    idx = np.arange(len(labels))
    test = np.zeros(0, np.int64)
    if test_split_ratio > 0:
        idx, test = _stratified_split(rng, idx, labels, test_split_ratio)
    train, val = _stratified_split(rng, idx, labels, 0.3)
    lim = math.sqrt(6.0 / (_lib.SI_EMBED + K))
    w0 = np.empty((restarts, _lib.SI_EMBED, K), np.float32)
    perm = np.empty((restarts, epochs, len(train)), np.int32)
    for r in range(restarts):
        rr = np.random.default_rng([int(seed), 1 + r])
        w0[r] = rr.uniform(-lim, lim, size=(_lib.SI_EMBED, K))
        for e in range(epochs):
            perm[r, e] = rr.permutation(len(train))
    r2 = np.random.default_rng([int(seed), 0, 2])
    perm2 = np.empty((int(fine_tune_epochs), len(train)), np.int32)
    for e in range(int(fine_tune_epochs)):
        perm2[e] = r2.permutation(len(train))
    return dict(train=train, val=val, test=test, w0=w0, b0=np.zeros((restarts, K), np.float32), perm=perm,
                perm2=perm2)


def fit_head(emb, labels, val_emb, val_labels, w0, b0, perm, epochs, batch=16, lr=1e-4, device=None):
    """Train Dense(K, sigmoid) heads on fixed embeddings, one kernel launch for the whole fit
    (``mmla_si_head_fit``: categorical_crossentropy + RMSprop as Keras 2.6 defines them, float32).
    emb [n,512], labels [n] class indices, val_* the validation set (None: none); w0 [R,512,K] /
    b0 [R,K] the initial head and perm [R,epochs,n] the sample order of each restart.
    -> (w [R,512,K], b [R,K], history [R,epochs,4] = loss, acc, val_loss, val_acc)."""
    ctx = _lib.default_context(device) if device is None or isinstance(device, int) else device
    return ctx.si_head_fit(emb, labels, val_emb, val_labels, w0, b0, perm, epochs, batch, lr)


HeadFit = namedtuple('HeadFit', 'w b accuracy history best test plan', defaults=(None,))


def fine_tune(W, K, x, labels, plan, epochs=20, batch=8, lr=1e-6, device=None):
    """Stage 2 of transfer_learning (:438-454) on the device (``mmla_si_finetune``): the whole network
    of the deployed tensors W (base + K-way sigmoid head) trainable under a fresh RMSprop(lr), `epochs`
    epochs of batch `batch` over the plan's training windows in the plan's stage-2 order (``perm2``),
    scored on its validation windows after every epoch.  x [n,256,39], labels [n] class indices.
    -> ({name: tensor} fine-tuned, history [epochs,4] = loss, acc, val_loss, val_acc).  The BatchNorm
    moving statistics are not trainable and come back bit-equal."""
    from . import weights
    ctx = _lib.default_context(device) if device is None or isinstance(device, int) else device
    x = np.asarray(x)
    labels = np.asarray(labels, dtype=np.int32)
    tr, va = plan['train'], plan['val']
    epochs = int(epochs)
    if epochs < 0 or len(plan['perm2']) < epochs:
        raise ValueError(f"{epochs} fine-tune epochs, the plan holds {len(plan['perm2'])} orders")
    out, hist = ctx.si_finetune(weights.pack(weights.SI, W, K), K, x[tr].astype(np.float32), labels[tr],
                                x[va].astype(np.float32), labels[va], plan['perm2'][:epochs], epochs, batch, lr)
    return weights.unpack(weights.SI, out, K), hist


_fine_tune = fine_tune      # transfer_learning's fine_tune= keyword shadows the function's name


def fine_tune_accuracy(history, plan):
    """model.evaluate after stage 2: the last epoch's val_acc (without a validation set: its acc)"""
    return float(history[-1, 3] if len(plan['val']) else history[-1, 1])


def fit_registration(emb, labels, K, seed, test_split_ratio, epochs, restarts, device=None,
                     fine_tune_epochs=0):
    """The part of a registration behind the embeddings, shared by transfer_learning and Room.register:
    the plan drawn from `seed` (``_fit_plan``), `restarts` heads fitted side by side (``fit_head``) and
    the choice between them -- the best final validation accuracy, ties by the lower validation loss,
    then the lower index (without a validation set: the training figures).  emb [n,512], labels [n].
    -> HeadFit(w [512,K], b [K] of the kept restart, its accuracy, history [R,epochs,4], the kept
    restart's index, the test split's indices, the plan; with fine_tune_epochs > 0 the plan also holds
    stage 2's orders, which changes nothing else)."""
    emb = np.asarray(emb)
    labels = np.asarray(labels, dtype=np.int32)
    plan = _fit_plan(labels, K, seed, test_split_ratio, epochs, restarts, fine_tune_epochs)
    tr, va = plan['train'], plan['val']
    w, b, hist = fit_head(emb[tr], labels[tr], emb[va], labels[va], plan['w0'], plan['b0'],
                          plan['perm'], epochs, batch=16, lr=1e-4, device=device)
    last = hist[:, -1]
    score = last[:, 2:] if len(va) else last[:, :2]      # (loss, acc) deciding between restarts
    best = min(range(restarts), key=lambda r: (-score[r, 1], score[r, 0], r))
    return HeadFit(w[best], b[best], float(score[best, 1]), hist, best, plan['test'], plan)


def deployed_weights(base_W, w, b):
    """the tensors of the deployed model: the base below its Dense head + the head (w [512,K], b [K])"""
    from . import weights
    K = int(np.shape(w)[1])
    head = weights.si_spec(K)[-2][0].rsplit('/', 1)[0]
    W = {n: base_W[n] for n, _, _ in weights.si_spec(K)[:-2]}
    W[head + '/kernel'] = w
    W[head + '/bias'] = b
    return W


def transfer_learning(_x, _y, seed, _test_split_ratio, base_model_path, final_model_path, *,
                      epochs=500, restarts=1, allow_synthetic=False, device=None, fine_tune=False,
                      fine_tune_epochs=20):
    """speaker_identification.py:401-477.  Stage 1: freeze the base model below its Dense head, fit
    Dense(dim, sigmoid, name='customized_dense') on the registration windows (500 epochs, batch 16,
    RMSprop 1e-4), save the deployed model to final_model_path and return its accuracy (on the test
    split when _test_split_ratio > 0, else on the validation split, as the reference).  The base runs
    once (``si_embed``), the whole fit is one kernel launch; `restarts` heads are trained side by side
    and the one with the best final validation accuracy (ties: lower validation loss) is kept.

    Stage 2 (:438-454) is opt-in, ``fine_tune=True``: the kept restart's head plus the base go through
    `fine_tune_epochs` epochs (the reference: 20) of RMSprop at 1e-6, batch 8, with the whole network
    trainable (``fine_tune`` / ``mmla_si_finetune``: BatchNorm on its moving statistics, the l2 penalties
    of res units 5, 6, 8, 9 in the loss); the saved bundle then holds the fine-tuned tensors and the
    returned accuracy is stage 2's final val_acc (with a test split: the deployed model's accuracy on
    it, as before).  With ``fine_tune=False`` (the default) stage 2 is not run and the saved base
    tensors equal the loaded ones bit for bit.  Splits, initial head and shuffles come from numpy
    (``_fit_plan``), not from sklearn / TensorFlow streams."""
    from . import models, tfbundle, weights
    _x = np.asarray(_x)
    _y = np.asarray(_y)
    if _y.ndim != 2 or len(_y) != len(_x) or len(_y) == 0:
        raise ValueError(f'_y {_y.shape}: expected one one-hot row per window of _x {_x.shape}')
    bad = np.flatnonzero(~(((_y == 0) | (_y == 1)).all(axis=1) & (_y.sum(axis=1) == 1)))
    if bad.size:
        raise ValueError(f'_y row {int(bad[0])} is not one-hot: {_y[bad[0]]}')
    K = int(np.unique(_y, axis=0).shape[0])
    labels = _y.argmax(axis=1).astype(np.int32)
    if labels.max() >= K:
        raise ValueError(f'_y names class {int(labels.max())} but holds only {K} distinct rows')
    if epochs < 1 or restarts < 1:
        raise ValueError('epochs and restarts must be >= 1')
    ft_epochs = int(fine_tune_epochs) if fine_tune else 0
    if ft_epochs < 0:
        raise ValueError('fine_tune_epochs must be >= 0')
    if fine_tune and K > _lib.SI_TRAIN_MAX_CLASSES:
        raise ValueError(f'{K} speakers: fine-tuning fits at most {_lib.SI_TRAIN_MAX_CLASSES}')
    base = models.load_model(base_model_path, kind=weights.SI, device=device,
                             allow_synthetic=allow_synthetic)
    base._ensure_loaded()
    emb = base.ctx.si_embed(_x)
    fit = fit_registration(emb, labels, K, seed, _test_split_ratio, epochs, restarts, base.ctx, ft_epochs)
    te = fit.test
    W = deployed_weights(base.W, fit.w, fit.b)
    accuracy = fit.accuracy
    if ft_epochs > 0:
        W, history = _fine_tune(W, K, _x, labels, fit.plan, ft_epochs, device=base.ctx)
        accuracy = fine_tune_accuracy(history, fit.plan)
    os.makedirs(final_model_path, exist_ok=True)
    tfbundle.save_deployed(final_model_path, W, K)
    if len(te):      # model.evaluate(x_test, y_test) on the model just saved
        deployed = models.load_model(final_model_path, device=base.ctx)
        accuracy = float((deployed.predict(_x[te]).argmax(axis=1) == labels[te]).mean())
        print('Accuracy on test set: ', accuracy)
    return accuracy


def transfer_learning_on_experiment(root_dir, **kw):
    """speaker_identification.py:480-503 with root_dir in the place of the script's Root_Dir: features
    of root_dir/experiment/corpus -> experiment/experiment_feature.npz + speaker_id_dict.json ->
    transfer_learning(x, y, 1, 0, root_dir/timit/model, root_dir/experiment/model).  Keyword arguments
    go to transfer_learning."""
    import json
    root_dir = str(root_dir)
    wav_files = get_wav_files(root_dir + '/experiment/corpus/')
    print(wav_files)
    x, y, speaker_id = make_feature_experiment(wav_files, device=kw.get('device'))
    np.savez(root_dir + '/experiment/experiment_feature', x, y)
    with open(root_dir + '/experiment/speaker_id_dict.json', 'w') as f:
        json.dump(speaker_id, f)
    input_feature = np.load(root_dir + '/experiment/experiment_feature.npz', allow_pickle=True)
    x = input_feature['arr_0']
    y = input_feature['arr_1']
    final_model_path = root_dir + '/experiment/model'
    if not os.path.exists(final_model_path):
        os.mkdir(final_model_path)
    return transfer_learning(x, y, 1, 0, root_dir + '/timit/model', final_model_path, **kw)


def res_model(input_shape=(256, 39), n_classes=630, seed=0, device=None):
    """speaker_identification.py:115-219: the untrained base network, a ``SpeakerIdModel`` with a softmax
    head on the Keras initial state (``weights.initial``: the initialisers' distributions with numpy's
    draws, not TensorFlow's).  input_shape must be the (256, 39) of the feature functions."""
    from . import models, weights
    if tuple(input_shape) != (_lib.SI_FRAMES, _lib.SI_DIMS):
        raise ValueError(f'input_shape {tuple(input_shape)}: the network is built for (256, 39)')
    n_classes = int(n_classes)
    if not 1 <= n_classes <= _lib.SI_BASE_MAX_CLASSES:
        raise ValueError(f'{n_classes} classes outside [1, {_lib.SI_BASE_MAX_CLASSES}]')
    return models.SpeakerIdModel(weights.initial(weights.SI, seed, n_classes), n_classes, _lib.HEAD_SOFTMAX,
                                 device=device)


HISTORY_KEYS = ('loss', 'categorical_accuracy', 'val_loss', 'val_categorical_accuracy')


class History:
    """What ``model.fit`` returns, as far as the reference reads it (:530-551): ``history`` is a dict of
    the four Keras keys, one value per epoch run.  ``epochs_run`` and ``best_epoch`` (0-based, None if no
    checkpoint was taken) say what the two callbacks did."""

    def __init__(self, rows, epochs_run, best_epoch):
        rows = np.asarray(rows, np.float32)[:epochs_run]
        self.history = {k: [float(v) for v in rows[:, i]] for i, k in enumerate(HISTORY_KEYS)}
        self.epoch = list(range(epochs_run))
        self.epochs_run = int(epochs_run)
        self.best_epoch = None if best_epoch < 0 else int(best_epoch)


def _one_hot_labels(y, what):
    y = np.asarray(y)
    if y.ndim != 2 or len(y) == 0:
        raise ValueError(f'{what} {y.shape}: expected one one-hot row per window')
    bad = np.flatnonzero(~(((y == 0) | (y == 1)).all(axis=1) & (y.sum(axis=1) == 1)))
    if bad.size:
        raise ValueError(f'{what} row {int(bad[0])} is not one-hot')
    return y.argmax(axis=1).astype(np.int32)


def train(x_train, y_train, x_validate, y_validate, *, epochs=200, batch_size=32, lr=1e-4, patience=10,
          checkpoint_path=None, checkpoint_period=10, seed=0, device=None):
    """speaker_identification.py:221-250 on the device (``mmla_si_base_train``): ``res_model`` trained from
    its initial state with RMSprop(lr), categorical cross-entropy, batch_size windows a step, for at most
    `epochs` epochs under EarlyStopping(val_loss, patience) and ModelCheckpoint(val_categorical_accuracy,
    save_best_only, mode 'max', period=checkpoint_period).  y is one-hot as the reference passes it; the
    class count is y_train.shape[1].  -> (model, history): the model holds the LAST epoch's weights (no
    restore_best_weights), is installed on the device and answers predict / predict_wavs at once;
    history.history is the dict the reference plots, history.best_epoch the checkpointed epoch.  With
    checkpoint_path the best weights are saved there in the base layout (``tfbundle.save_speaker_base``)
    when a checkpoint was taken.  Everything random comes from `seed` through numpy: the initial state
    (``weights.initial``), the order of every epoch and the dropout seed; TensorFlow's streams are not
    reproduced."""
    from . import models, tfbundle, weights
    x_train = np.asarray(x_train)
    labels = _one_hot_labels(y_train, 'y_train')
    K = int(np.shape(y_train)[1])
    if len(x_train) != len(labels):
        raise ValueError(f'x_train {x_train.shape}: expected one window per row of y_train')
    nv = 0 if x_validate is None else len(x_validate)
    vx = vl = None
    if nv:
        vl = _one_hot_labels(y_validate, 'y_validate')
        if np.shape(y_validate)[1] != K or len(vl) != nv:
            raise ValueError(f'y_validate {np.shape(y_validate)}: expected [{nv},{K}]')
        vx = np.asarray(x_validate).astype(np.float32)
    epochs = int(epochs)
    if epochs < 0 or batch_size < 1:
        raise ValueError('epochs must be >= 0 and batch_size >= 1')
    model = res_model(x_train.shape[1:], K, seed, device)
    rng = np.random.default_rng([int(seed), 3])
    drop_seed = int(rng.integers(0, 2 ** 63))
    perm = np.empty((epochs, len(labels)), np.int32)
    for e in range(epochs):
        perm[e] = rng.permutation(len(labels))
    period = int(checkpoint_period)
    out, best, hist, ran, best_ep = model.ctx.si_base_train(
        weights.pack(weights.SI, model.W, K), K, x_train.astype(np.float32), labels, vx, vl, perm, epochs,
        batch_size, lr, drop_seed, patience, period)
    model.set_weights(weights.unpack(weights.SI, out, K), K, _lib.HEAD_SOFTMAX)
    if checkpoint_path is not None and best is not None:
        os.makedirs(checkpoint_path, exist_ok=True)
        tfbundle.save_speaker_base(checkpoint_path, weights.unpack(weights.SI, best, K), K)
    return model, History(hist, ran, best_ep)


def make_feature_timit(wav_files, speaker_ids, data_dir, device=None, chunk=256):
    """speaker_identification.py:264-314 with data_dir in the place of Root_Dir + '/timit/data': per file
    the MFCC + delta + delta-delta features of the whole recording, zero-padded or cut to 256 frames, and
    the one-hot speaker rows of ``binarizer(dim=630)`` -> (x float64 [n,256,39], y [n,630]).  wav_files
    and speaker_ids are sequences (or pandas columns, as the reference passes them); device: a device
    index or a ``_lib.Context``.  Unlike
    ``input_feature_gen`` there is no 'silent' rule here: a recording below 4000 samples gets its
    features like any other, as in the reference.  Features run `chunk` files at a time on the device
    (``input_feature_batch``'s call; a recording below that length goes through ``si_features_seq``)."""
    wav_files = list(getattr(wav_files, 'values', wav_files))
    speaker_ids = list(getattr(speaker_ids, 'values', speaker_ids))
    if len(wav_files) != len(speaker_ids):
        raise ValueError(f'{len(wav_files)} files, {len(speaker_ids)} speaker ids')
    ctx = _lib.default_context(device) if device is None or isinstance(device, int) else device
    xs = []
    for i0 in range(0, len(wav_files), int(chunk)):
        sigs = [_read(os.path.join(str(data_dir), str(f))) for f in wav_files[i0:i0 + int(chunk)]]
        feat, silent = ctx.si_features(sigs)
        for j in np.flatnonzero(silent):      # below the 'silent' length: the whole-signal path, window 0
            feat[j] = ctx.si_features_seq(sigs[j])[0] if len(sigs[j]) else 0.0
        xs.append(feat.astype(np.float64))
    y = binarizer(speaker_ids, dim=630)
    x = np.concatenate(xs) if xs else np.zeros((0, _lib.SI_FRAMES, _lib.SI_DIMS))
    return x, np.asarray(y)


def conversation_features(sig, device=None):
    """Whole-sequence MFCC + deltas cut into 256-frame windows -> float64 [S, 256, 39]
    (speaker_identification_post_processing.py:255-269; make_feature_experiment :341-353)."""
    return _lib.default_context(device).si_features_seq(np.asarray(sig, np.int16)).astype(np.float64)
