"""GPU (-m gpu): every refusal of the six online solve entry points (trmf_session_assimilate, _assimilate_robust, _smooth,
_smooth_robust, _series_stats_init / _adapt_series, _adapt_series_robust; csrc/trmf_abi.hip), with its FULL message.  One table:
the session the call meets, the call, the message as a literal -- written out here, not put together from the library's helpers,
so that a check that moves, a message that changes by a word or a check that is lost shows.  After each refusal the downloaded W
and H are the bits they were.  No call in here solves anything (a pivot failure is provoked numerically by test_gpu_online.py and
its siblings): the sessions are the online_helpers case at rank 16, and a rank-65 session of 32 rows for the rank refusal."""
import numpy as np
import pytest

import online_helpers as OH
from helpers import make_model
from trmf.session import Session

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
IDS = ['float32', 'float64']
K = 16
BAD = 3                                                     # the series whose scale is zero

RANK = '{}: online updates cover the register-tiled ranks 1..64, this session has rank 65'
LAG0 = '{}: the lag set contains lag 0 (a row would be its own prior)'
FIRST_LOW = '{}: first_row 4 outside [5 (the largest lag), 96 (rows)]'
FIRST_HIGH = '{}: first_row 97 outside [5 (the largest lag), 96 (rows)]'
CAP = '{}: a window of 24 rows is above the cap of 23 rows (the factors of every window row stay resident for the solve)'
RTOL = '{}: rtol must be finite (<= 0: the default of the element type)'
MAX_ITER = '{}: max_iter 16384 above 16383'
SWEEPS_0 = '{}: sweeps 0 outside 1..64'
SWEEPS_65 = '{}: sweeps 65 outside 1..64'
NO_SCALE = '{}: no scale given and no noise fitted or set (trmf_session_fit_noise / _set_noise)'
SCALE_GIVEN = '{}: the scale of series 3 is not finite and positive'
SCALE_RESIDENT = '{}: the scale of series 3 is not finite and positive (the square root of the resident sigma2)'
NO_SLOT = ('{}: sparse storage with missing == 0 is not covered (an absent entry there is an observation without a slot to report its '
           'weight in); store the matrix dense')
NO_STATS = '{}: no series statistics (trmf_session_series_stats_init first)'
STALE = ('{}: the series statistics are stale: rows they absorbed may have changed (run, rewind, assimilate below the absorbed rows, or a '
         'new series transform); initialise them again (trmf_session_series_stats_init)')
ONE_S = ('adapt_series_robust: {} is a full-observation form: it keeps ONE shared S for all series, and a weight per cell needs a table '
         'per series (sparse storage with missing != 0); use adapt_series')


def _zero_scale():
    sc = np.full(OH.N, 0.3)
    sc[BAD] = 0.0
    return sc


def _robust(name, plain):
    """The refusals the three Huber calls share; `plain`: what c == infinity is called in this call's message."""
    call = lambda **kw: (lambda s: getattr(s, name)(*(() if name == 'adapt_series_robust' else (OH.FIRST,)), **dict(dict(scale=0.3), **kw)))
    home = 'stats' if name == 'adapt_series_robust' else 'sparse'
    return [
        ('c zero', home, call(c=0.0), '{}: c must be positive (infinity: ' + plain + ')'),
        ('c nan', home, call(c=float('nan')), '{}: c must be positive (infinity: ' + plain + ')'),
        ('sweeps 0', home, call(sweeps=0), SWEEPS_0),
        ('sweeps 65', home, call(sweeps=65), SWEEPS_65),
        ('no scale, no noise', home, call(scale=None), NO_SCALE),
        ('scale given zero', home, call(scale=_zero_scale()), SCALE_GIVEN),
        ('scale resident zero', home + '+noise0', call(scale=None), SCALE_RESIDENT),
    ]


def _windowed(name, **kw):
    """The refusals the two smoothers share."""
    call = lambda first=OH.FIRST, **more: (lambda s: getattr(s, name)(first, **dict(kw, **more)))
    return [
        ('window cap', 'sparse', call(), CAP),
        ('rtol nan', 'sparse', call(rtol=float('nan')), RTOL),
        ('rtol inf', 'sparse', call(rtol=float('inf')), RTOL),
        ('max_iter 16384', 'sparse', call(max_iter=16384), MAX_ITER),
    ]


def _rows(name, **kw):
    """The refusals the four calls over a range of rows share."""
    call = lambda first=OH.FIRST: (lambda s: getattr(s, name)(first, **kw))
    return [
        ('rank 65', 'rank65', call(20), RANK),
        ('lag 0', 'lag0', call(), LAG0),
        ('first_row below the largest lag', 'sparse', call(4), FIRST_LOW),
        ('first_row above rows()', 'sparse', call(OH.T + 1), FIRST_HIGH),
    ]


# call -> [(refusal, the session it meets, the call, the message with {} for the call's name)]
TABLE = {
    'assimilate': _rows('assimilate'),
    'assimilate_robust': _rows('assimilate_robust', scale=0.3) + [
        ('sparse storage, missing == 0', 'sparse_full', lambda s: s.assimilate_robust(OH.FIRST, scale=0.3), NO_SLOT),
    ] + _robust('assimilate_robust', 'the plain filter'),
    'smooth': _rows('smooth') + _windowed('smooth'),
    'smooth_robust': _rows('smooth_robust', scale=0.3) + [
        ('sparse storage, missing == 0', 'sparse_full', lambda s: s.smooth_robust(OH.FIRST, scale=0.3), NO_SLOT),
    ] + _windowed('smooth_robust', scale=0.3) + _robust('smooth_robust', "the plain smoother's objective"),
    'series_stats_init': [
        ('rank 65', 'rank65', lambda s: s.init_series_stats(), RANK),
        ('forget zero', 'sparse', lambda s: s.init_series_stats(0.0), '{}: forget must lie in (0, 1]'),
        ('forget above one', 'sparse', lambda s: s.init_series_stats(1.5), '{}: forget must lie in (0, 1]'),
        ('forget nan', 'sparse', lambda s: s.init_series_stats(float('nan')), '{}: forget must lie in (0, 1]'),
    ],
    'adapt_series': [
        ('rank 65', 'rank65', lambda s: s.adapt_series(), RANK),
        ('no statistics', 'sparse', lambda s: s.adapt_series(), NO_STATS),
        ('stale statistics', 'stale', lambda s: s.adapt_series(), STALE),
    ],
    'adapt_series_robust': [
        ('rank 65', 'rank65', lambda s: s.adapt_series_robust(scale=0.3), RANK),
        ('dense storage', 'dense', lambda s: s.adapt_series_robust(scale=0.3), ONE_S.format('dense storage')),
        ('sparse storage, missing == 0', 'sparse_full', lambda s: s.adapt_series_robust(scale=0.3), ONE_S.format('sparse storage with missing == 0')),
        ('no statistics', 'sparse', lambda s: s.adapt_series_robust(scale=0.3), NO_STATS),
        ('stale statistics', 'stale', lambda s: s.adapt_series_robust(scale=0.3), STALE),
    ] + _robust('adapt_series_robust', 'the plain update'),
}
CASES = [(name,) + row for name, rows in TABLE.items() for row in rows]


def _open(kind, dtype):
    """(session, W, H as uploaded) of one kind: the storage, the lag set, the rank and the state of the tables a refusal needs."""
    base, _, state = kind.partition('+')
    d = OH.inputs(K)
    W, H, theta, lags, Y = d['W'], d['H'], d['theta'], d['lag_set'], d['Y'].astype(dtype)
    missing = base not in ('dense', 'sparse_full')
    if base == 'dense':
        Y = np.ascontiguousarray(Y.toarray())
    elif base == 'lag0':
        lags = np.array([0, 1, 5], dtype=np.uint32)
    elif base == 'rank65':
        rng = np.random.RandomState(5)
        W, H, Y = rng.rand(32, 65), rng.rand(20, 65), Y[:32, :20]
        theta = np.asfortranarray(0.2 * rng.randn(3, 65))
    model = make_model(np.ascontiguousarray(W.astype(dtype)), np.ascontiguousarray(H.astype(dtype)), np.asfortranarray(theta.astype(dtype)), lags)
    W0, H0 = model.W.copy(), model.H.copy()
    s = Session(Y, model, lambdaI=0.5, lambdaAR=50.0, lambdaLag=0.5, missing=missing)
    if base in ('stats', 'stale'):
        s.init_series_stats(1.0)
    if base == 'stale':                                     # a rewind to the state the session is in: the tables go stale, nothing moves
        s.mark().rewind()
    if state == 'noise0':
        sigma2 = np.full(OH.N, 0.09)
        sigma2[BAD] = 0.0
        s.set_noise(sigma2, np.full(K, 0.01))
    return s, W0, H0


@pytest.fixture(scope='module')
def sessions():
    held = {}

    def get(kind, dtype):
        key = (kind, np.dtype(dtype).name)
        if key not in held:
            held[key] = _open(kind, dtype)
        return held[key]
    yield get
    for s, _, _ in held.values():
        s.close()


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('name,refusal,kind,call,message', CASES, ids=['%s: %s' % c[:2] for c in CASES])
def test_a_refused_call_names_its_reason_in_full_and_changes_nothing(name, refusal, kind, call, message, dtype, sessions, monkeypatch):
    s, W0, H0 = sessions(kind, dtype)
    if refusal == 'window cap':
        monkeypatch.setenv('TRMF_SMOOTH_MAX_ROWS', '23')
    with pytest.raises(RuntimeError) as err:
        call(s)
    assert str(err.value) == 'trmf_session_%s failed: %s' % (name, message.format(name))
    model = s.download()
    assert np.array_equal(model.W, W0) and np.array_equal(model.H, H0)
