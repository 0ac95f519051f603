"""Weight layouts of the two reference networks, seeded synthetic weights, and packing for the C-ABI.

The trained weights are absent from the reference (``.MISSING_LARGE_BLOBS:1-6``), so parity runs on
seeded synthetic weights laid out exactly like the reference ``variables.index`` files
(SURVEY.md 8a "Weight layouts").  ``mmla_audio_amd.tfbundle.load_bundle`` loads the real ones the
moment the data shard is supplied.

Canonical names are the bundle's ``layer_with_weights-<k>/<var>``; the Bidirectional LSTM's six
tensors are ``layer_with_weights-<k>/{forward,backward}/{kernel,recurrent_kernel,bias}``.

OD (``OverlapDetection/timit/models/timit2.0``): lww-0 stem Conv2D [1,1,3,16]; per res_block
``BN, Conv3x3, BN, Conv(4,1)[, shortcut Conv1x1/2]`` through lww-39; lww-40 BiLSTM(256) on 128
inputs; lww-41 Dense [512,2].
SI (``SpeakerIdentification/timit/model``): lww-0 Conv1D [4,39,32]; per res_unit
``BN, Conv3, BN[, shortcut Conv1/2], Conv3`` through lww-39; lww-40 final BN128; lww-41 BiLSTM;
lww-42 Dense [512,K] (K=630 softmax base model, or the deployed ``customized_dense`` sigmoid head,
``speaker_identification.py:409``).

The packed order handed to ``mmla_load_weights`` is the order of ``spec()``: ascending layer index;
conv/dense = kernel, bias; BN = gamma, beta, moving_mean, moving_variance; BiLSTM = forward kernel,
recurrent_kernel, bias, backward kernel, recurrent_kernel, bias.  Arrays keep the Keras layouts
(Conv2D [kh,kw,cin,cout], Conv1D [k,cin,cout], Dense [in,out], LSTM [in,4u] gates i,f,c,o).
"""
import numpy as np

OD = 0
SI = 1
CHANNELS = (32, 32, 32, 64, 64, 64, 128, 128, 128)
POOL = (True, False, False, True, False, False, True, False, False)
LSTM_UNITS = 256


def _bn(k, c):
    p = f'layer_with_weights-{k}/'
    return [(p + 'gamma', (c,), 'bn_gamma'), (p + 'beta', (c,), 'bn_beta'),
            (p + 'moving_mean', (c,), 'bn_mean'), (p + 'moving_variance', (c,), 'bn_var')]


def _conv(k, shape):
    p = f'layer_with_weights-{k}/'
    return [(p + 'kernel', tuple(shape), 'kernel'), (p + 'bias', (shape[-1],), 'bias')]


def _bilstm(k, d):
    out = []
    for side in ('forward', 'backward'):
        p = f'layer_with_weights-{k}/{side}/'
        out += [(p + 'kernel', (d, 4 * LSTM_UNITS), 'lstm_kernel'),
                (p + 'recurrent_kernel', (LSTM_UNITS, 4 * LSTM_UNITS), 'lstm_rec'),
                (p + 'bias', (4 * LSTM_UNITS,), 'lstm_bias')]
    return out


OD_MAX_CLASSES = 8   # MMLA_OD_MAX_CLASSES


OD_CHANNELS = (3, 1)   # the stem's input channels: RGB images, or OverlapDetector(imagetype='gray')


def od_spec(n_classes=2, channels=3):
    """[(name, shape, role)] in packed order for OD-NET with a K-way head (its last item; 2: the deployed
    timit2.0 model, 3: the reference's research models, overlap_detector.py:394) on images of `channels`
    channels (3; 1: imagetype='gray', whose stem is Conv2D(16, 1) on one channel, overlap_detector.py:84-90)."""
    if not 2 <= int(n_classes) <= OD_MAX_CLASSES:
        raise ValueError(f'OD n_classes {n_classes} outside [2, {OD_MAX_CLASSES}]')
    if int(channels) not in OD_CHANNELS:
        raise ValueError(f'OD channels {channels}: expected 3 or 1')
    s = _conv(0, (1, 1, int(channels), 16))
    k = 1
    cin = 16
    for c, pool in zip(CHANNELS, POOL):
        s += _bn(k, cin) + _conv(k + 1, (3, 3, cin, c)) + _bn(k + 2, c) + _conv(k + 3, (4, 1, c, c))
        if pool:
            s += _conv(k + 4, (1, 1, cin, c))
            k += 5
        else:
            k += 4
        cin = c
    s += _bilstm(40, 128)
    s += _conv(41, (512, int(n_classes)))
    return s


def si_spec(n_classes=630):
    """[(name, shape, role)] in packed order for SI-NET with a K-way head."""
    s = _conv(0, (4, 39, 32))
    k = 1
    cin = 32
    for c, pool in zip(CHANNELS, POOL):
        s += _bn(k, cin) + _conv(k + 1, (3, cin, c)) + _bn(k + 2, c)
        if pool:
            s += _conv(k + 3, (1, cin, c)) + _conv(k + 4, (3, c, c))
            k += 5
        else:
            s += _conv(k + 3, (3, c, c))
            k += 4
        cin = c
    s += _bn(40, 128)
    s += _bilstm(41, 128)
    s += _conv(42, (512, n_classes))
    return s


def spec(kind, n_classes=None, channels=3):
    if kind == OD:
        return od_spec(2 if n_classes is None else n_classes, channels)
    return si_spec(630 if n_classes is None else n_classes)


def _glorot(rng, shape):
    if len(shape) == 2:
        fan_in, fan_out = shape
    else:
        rf = int(np.prod(shape[:-2]))
        fan_in, fan_out = rf * shape[-2], rf * shape[-1]
    lim = np.sqrt(6.0 / (fan_in + fan_out))
    return rng.uniform(-lim, lim, size=shape), fan_in, lim * lim / 3.0


def _orthogonal(rng, shape):
    a = rng.standard_normal((shape[1], shape[0]))
    q, r = np.linalg.qr(a)
    q = q * np.sign(np.diag(r))
    return q.T


SI_HEAD_GAIN = 10.0   # synthetic SI Dense kernel scale: decisive argmax at K = 630 (logit std ~4)


def od_classes_of(n_floats):
    """K of a packed OD blob of n_floats = (the blob below the head) + 513 K; ValueError for any other size."""
    k, rest = divmod(int(n_floats) - (n_params(OD) - 513 * 2), 513)
    if rest or not 2 <= k <= OD_MAX_CLASSES:
        raise ValueError(f'{n_floats} floats is not an OD blob of 2..{OD_MAX_CLASSES} classes')
    return k


def od_layout_of(n_floats):
    """(K, channels) of a packed OD blob of n_floats.  A one-channel blob is 32 floats (two rows of the stem
    kernel) shorter than the three-channel blob of its K, and 513 K - 32 is no multiple of 513: no two
    layouts share a size.  ValueError for any other size."""
    base = n_params(OD) - 513 * 2
    for ch in OD_CHANNELS:
        k, rest = divmod(int(n_floats) - base + (32 if ch == 1 else 0), 513)
        if not rest and 2 <= k <= OD_MAX_CLASSES:
            return k, ch
    raise ValueError(f'{n_floats} floats is not an OD blob of 2..{OD_MAX_CLASSES} classes and 3 or 1 channels')


def od_classes(W):
    """K of an OD weight dict: the width of its Dense head."""
    return int(W['layer_with_weights-41/kernel'].shape[1])


def od_channels(W):
    """Input channels of an OD weight dict: the stem kernel's [1,1,C,16]."""
    return int(W['layer_with_weights-0/kernel'].shape[2])


def synthetic(kind, seed=0, n_classes=None, head_gain=None, channels=3):
    """Seeded synthetic weights in the reference layout.

    Kernels are Glorot-uniform (the Keras default the reference trains from), recurrent kernels
    orthogonal, LSTM biases ``unit_forget_bias``.  BatchNorm moving statistics are not the
    Keras initial (0, 1): they are set from a second-moment estimate propagated through the graph
    so that every BN actually normalises, as a trained model's would, and the stem kernel is scaled
    for the input range (0..255 PNG values for OD, MFCC magnitudes for SI).  All non-zero, so every
    fused bias / BN / residual term is exercised by parity tests.  The SI head's Dense kernel is
    scaled by ``head_gain`` (default SI_HEAD_GAIN): Glorot alone gives logits with std ~0.4 over 630
    classes, a nearly flat softmax a trained classifier would not produce and on which argmax checks
    decide little.
    """
    rng = np.random.default_rng(np.random.PCG64(0x6D6D6C61 + 7919 * seed + 31 * kind))
    W = {}
    m2 = 2.0e4 if kind == OD else 150.0     # second moment of the network input
    stem_gain = None
    act_m2 = 0.6                              # E[act(bn(x))^2] for unit-variance BN output
    items = spec(kind, n_classes, channels)
    i = 0
    cur = m2
    resid = None
    while i < len(items):
        name, shape, role = items[i]
        if role == 'kernel':
            w, fan_in, var_w = _glorot(rng, shape)
            if stem_gain is None:
                stem_gain = 1.0 / np.sqrt(fan_in * var_w * m2)
                w = w * stem_gain
                var_w = var_w * stem_gain ** 2
            W[name] = w
            b_name = items[i + 1][0]
            W[b_name] = rng.uniform(-0.05, 0.05, size=items[i + 1][1])
            cur = fan_in * var_w * cur + 0.05 ** 2 / 3
            i += 2
            continue
        if role == 'bn_gamma':
            c = shape[0]
            W[name] = rng.uniform(0.8, 1.2, size=c)
            W[items[i + 1][0]] = rng.uniform(-0.1, 0.1, size=c)
            mean = rng.uniform(-0.1, 0.1, size=c) * np.sqrt(cur)
            W[items[i + 2][0]] = mean
            W[items[i + 3][0]] = cur * rng.uniform(0.8, 1.25, size=c)
            cur = act_m2
            i += 4
            continue
        if role == 'lstm_kernel':
            for j in range(2):
                kn, ks, _ = items[i + 3 * j]
                rn, rs, _ = items[i + 3 * j + 1]
                bn, bs, _ = items[i + 3 * j + 2]
                W[kn] = _glorot(rng, ks)[0]
                W[rn] = _orthogonal(rng, rs)
                b = rng.uniform(-0.05, 0.05, size=bs)
                b[LSTM_UNITS:2 * LSTM_UNITS] += 1.0
                W[bn] = b
            i += 6
            continue
        raise AssertionError(f'unexpected role {role} at {name}')
    del resid
    if head_gain is None:
        head_gain = SI_HEAD_GAIN if kind == SI else 1.0
    head = [n for n, _, r in items if r == 'kernel'][-1]
    W[head] = W[head] * head_gain
    return {k: np.asarray(v, dtype=np.float32) for k, v in W.items()}


def initial(kind, seed=0, n_classes=None):
    """The state a freshly built Keras model starts training from (``res_model``,
    speaker_identification.py:115-219), for SI: Glorot-uniform kernels, zero biases, gamma 1, beta 0,
    moving mean 0, moving variance 1, orthogonal recurrent kernels, LSTM bias 0 with the forget block 1
    (``unit_forget_bias``).  The draws are numpy's (PCG64 seeded by ``seed``): the initialisers'
    distributions are Keras's, TensorFlow's generator is not reproduced, so no seed gives TensorFlow's
    numbers.  OD-NET's initial state has a name of its own, ``initial_od``.
    """
    if kind != SI:
        raise NotImplementedError('weights.initial: only the SI network is trained from scratch')
    return _initial(spec(kind, n_classes), 0x696E6974 + 7919 * int(seed))


def initial_od(seed=0, n_classes=2, channels=3):
    """The Keras initial state of ``__ResBLSTM`` (overlap_detector.py:362-390), what ``train_model`` starts
    from: the same initialisers as ``initial`` over ``od_spec(n_classes)``, with numpy's draws from a stream
    of its own.  The head is the last draw, so every other tensor is the two-class draw bit for bit.
    channels=1: the one-channel stem of imagetype='gray' (the first draw, so the other tensors differ)."""
    return _initial(od_spec(n_classes, channels), 0x696E6F64 + 7919 * int(seed))


def _initial(items, stream):
    rng = np.random.default_rng(np.random.PCG64(stream))
    fixed = {'bias': 0.0, 'bn_gamma': 1.0, 'bn_beta': 0.0, 'bn_mean': 0.0, 'bn_var': 1.0}
    W = {}
    for name, shape, role in items:
        if role in ('kernel', 'lstm_kernel'):
            W[name] = _glorot(rng, shape)[0]
        elif role == 'lstm_rec':
            W[name] = _orthogonal(rng, shape)
        elif role == 'lstm_bias':
            b = np.zeros(shape)
            b[LSTM_UNITS:2 * LSTM_UNITS] = 1.0
            W[name] = b
        else:
            W[name] = np.full(shape, fixed[role])
    return {k: np.asarray(v, dtype=np.float32) for k, v in W.items()}


def check(kind, W, n_classes=None, channels=3):
    """Raise ValueError unless W has exactly the spec's names and shapes."""
    items = spec(kind, n_classes, channels)
    names = {n for n, _, _ in items}
    missing = [n for n in names if n not in W]
    if missing:
        raise ValueError(f'missing weights: {missing[:5]}...')
    for n, s, _ in items:
        if tuple(W[n].shape) != tuple(s):
            raise ValueError(f'{n}: shape {tuple(W[n].shape)} != expected {s}')


def pack(kind, W, n_classes=None, channels=3):
    """Flatten W into the canonical float32 blob for ``mmla_load_weights`` (channels: the OD stem's, 3 or 1)."""
    check(kind, W, n_classes, channels)
    return np.concatenate([np.ascontiguousarray(W[n], dtype=np.float32).ravel()
                           for n, _, _ in spec(kind, n_classes, channels)])


def unpack(kind, blob, n_classes=None, channels=3):
    """The inverse of ``pack``: the flat float32 blob -> {name: array} in the spec's shapes."""
    blob = np.asarray(blob, dtype=np.float32).ravel()
    items = spec(kind, n_classes, channels)
    if blob.size != sum(int(np.prod(s)) for _, s, _ in items):
        raise ValueError(f'blob of {blob.size} floats, the spec holds {n_params(kind, n_classes, channels)}')
    W, at = {}, 0
    for name, shape, _ in items:
        n = int(np.prod(shape))
        W[name] = blob[at:at + n].reshape(shape).copy()
        at += n
    return W


def n_params(kind, n_classes=None, channels=3):
    return int(sum(int(np.prod(s)) for _, s, _ in spec(kind, n_classes, channels)))
