"""Folding unseen entities into a trained vectorspace model (include/sert_hip_foldin.h).

A catalogue gains entities after training.  The LSE paper's answer is to fold them in: keep the word table, the
projection and the trained entity rows fixed and learn only the new rows, with the same NCE objective, on the new
entities' instances.  ``EntityFoldIn`` is that, on the device; ``bin/fold_in.py`` is its command line.

``LogLinearFoldIn`` is the same for a trained loglinear (expert-finding) model (include/sert_hip_ll_foldin.h): the word table
and the trained columns of the output layer stay fixed and the new entities' columns and biases learn.  With ``refresh`` the
columns and biases of trained entities that gained documents learn too (bin/fold_in.py --unfreeze_known).

``WordFoldIn`` is the other half of a catalogue that changes after training (include/sert_hip_wfold.h): the VOCABULARY grows.
The trained word rows, the projection and the whole entity table stay fixed and only the rows of the new words learn
(bin/prepare.py --extend_vocabulary, bin/fold_in.py --new_words).

``LogLinearWordFoldIn`` is the same for a trained loglinear model (include/sert_hip_ll_wfold.h): the trained word rows, W and b
stay fixed and the rows of the new words learn with the model's own loss (bin/fold_in.py --ll_new_words).
"""
import logging
import pickle

import numpy as np
import scipy.sparse

from sert_amd import _capi
from sert_amd import models


class _FoldInModel(models.ModelInterface):
    """What the four fold-in models share: one shuffled pass over the uploaded batches, the evaluation pass, and the life of
    the device handle ``_foldin`` (a ``_capi`` owner made from an engine that may be a throwaway)."""

    #: callable batch_index -> negatives, or None; only the NCE fold-ins have one
    negative_sampler = None
    #: batches issued to the device before their losses are read back (device-drawn negatives only)
    steps_per_sync = 1

    def _attach(self, engine, make_engine, make_handle):
        """``_foldin`` = make_handle(engine); engine None: a parameters-only model from make_engine() holds the frozen tensors
        on the device for the moment of the copy."""
        owned = engine is None
        if owned:
            engine = make_engine()
        try:
            self._foldin = make_handle(engine)
        finally:
            if owned:
                engine.close()      # (the handle copied what it needs)

    def train_fn(self, batch_index):
        return self._foldin.train_batch(batch_index)

    def test_fn(self, batch_index):
        return self._foldin.eval_batch(batch_index)

    def train(self):
        """One pass over the complete batches in shuffled order, as ModelBase.train: (num_batches, mean loss)."""
        count = self.training_num_instances
        logging.info('Folding in on %d instances (%d batches).', count, self._number_of_batches(count))
        if self.steps_per_sync > 1 and self.negative_sampler is None:
            num_batches, losses = self._iterate_chunks(self._foldin.train_batches, count, int(self.steps_per_sync),
                                                       report_interval=1000, shuffle=True)
        else:
            num_batches, losses = self._iterate_batches(self.train_fn, count, report_interval=1000, shuffle=True)
        return num_batches, np.mean(losses)

    def train_error(self):
        """(mean, std) of the per-batch evaluation losses on the extended model: unweighted, unregularised."""
        count = self.training_num_instances
        logging.info('Measuring error on %d fold-in instances (%d batches).', count, self._number_of_batches(count))
        _, losses = self._iterate_batches(self.test_fn, count)
        return np.mean(losses), np.std(losses)

    def close(self):
        self._foldin.close()


class _NceFoldInModel(_FoldInModel):
    """The two fold-ins of a vectorspace model on top of it: host-side negative samplers, Adam's and the device sampler's
    state, and the throwaway engine."""

    #: callable batch_index -> (B, z) int64 negatives in the range the handle draws from, or None (device sampler)
    negative_sampler = None
    #: same, for train_error()
    eval_negative_sampler = None
    #: the keys of Adam's moments in get_optimizer_state()
    _moment_keys = None

    @staticmethod
    def _vs_engine(R_w, R_e, W, b, window_size, device):
        """A parameters-only vectorspace model on the device that holds the frozen tensors."""
        R_w, R_e = np.asarray(R_w, dtype=np.float32), np.asarray(R_e, dtype=np.float32)
        W, b = np.asarray(W, dtype=np.float32), np.asarray(b, dtype=np.float32)
        assert W.shape == (R_w.shape[1], R_e.shape[1]) and b.shape == (R_e.shape[1],)
        engine = _capi.Engine(
            kind=_capi.KIND_VECTORSPACE, batch_size=1, global_batch_size=1, window_size=window_size,
            vocab_size=R_w.shape[0], num_entities=R_e.shape[0], word_dim=R_w.shape[1], entity_dim=R_e.shape[1],
            num_negatives=0, id_bytes=4, device=device, keep_grads=0, deterministic=1, inference_only=1, lambda_=0.0,
            lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, seed=0)
        for which, value in ((_capi.T_RW, R_w), (_capi.T_RE, R_e), (_capi.T_W, W), (_capi.T_B, b)):
            engine.set_tensor(which, value)
        return engine

    def train_fn(self, batch_index):
        sampler = self.negative_sampler
        return self._foldin.train_batch(batch_index, None if sampler is None else np.asarray(sampler(batch_index)))

    def test_fn(self, batch_index):
        sampler = self.eval_negative_sampler
        return self._foldin.eval_batch(batch_index, None if sampler is None else np.asarray(sampler(batch_index)))

    def get_optimizer_state(self):
        m, v = self._moment_keys
        return {'step': self._foldin.get_step(), m: self._foldin.get_rows(_capi.FOLDIN_M), v: self._foldin.get_rows(_capi.FOLDIN_V)}

    def set_optimizer_state(self, st):
        m, v = self._moment_keys
        self._foldin.set_step(st['step'])
        self._foldin.set_rows(_capi.FOLDIN_M, st[m])
        self._foldin.set_rows(_capi.FOLDIN_V, st[v])

    def get_sampler_state(self):
        return {'seed': int(self._foldin.cfg.seed), 'eval_draws': self._foldin.get_eval_draws()}

    def set_sampler_state(self, st):
        if int(st['seed']) != int(self._foldin.cfg.seed):
            raise RuntimeError('the sampler seed is fixed at construction')
        self._foldin.set_eval_draws(st['eval_draws'])


class EntityFoldIn(_NceFoldInModel):
    """N new entity rows learnt on top of a trained vectorspace model (R_w, R_e, W, b: host arrays, never written).

    training_set: (x (M, window_size) token ids of the TRAINED vocabulary, y (M,) in [0, N), w (M,) weights or None).
    New entity e becomes row V_e + e of the extended table.  ``new_rows_init`` None: N = y.max() + 1 rows drawn with
    ``_glorot_uniform((N, d_e))``, as bin/train.py initialises R_e.  The batch size, the number of negatives, lambda and the
    learning rate are the fold-in's own.

    ``refresh`` (an array of distinct trained internal indices): these trained rows learn too -- entities that gained
    documents.  The trainable rows are then SLOTS, the refreshed rows first, in the order of ``refresh``, the new rows
    behind them: y is a slot in [0, len(refresh) + N), and ``new_rows_init`` may be None or empty (nothing is new).
    Negatives stay ids of the extended table.  A refreshed row starts from its trained value and learns from the
    instances given: to keep its old evidence, pass the entity's old documents along with the new ones."""

    #: negative_sampler / eval_negative_sampler draw from [0, V_e + N)
    _moment_keys = ('m_E', 'v_E')

    def __init__(self, R_w, R_e, W, b, new_rows_init, training_set, batch_size, num_negative_samples,
                 regularization_lambda, window_size, seed=None, lr=1e-3, device=0, _engine=None, refresh=None):
        super(EntityFoldIn, self).__init__(batch_size)
        x, y = np.asarray(training_set[0]), np.asarray(training_set[1])
        w = training_set[2] if len(training_set) > 2 else None
        assert x.ndim == 2 and x.shape[1] == window_size and y.ndim == 1 and y.shape[0] == x.shape[0]
        if refresh is not None:
            refresh = np.asarray(refresh, dtype=np.int64).reshape(-1)
            if new_rows_init is None:
                new_rows_init = np.zeros((0, np.shape(R_e)[1]), dtype=np.float32)
        if new_rows_init is None:
            if not y.size:
                raise RuntimeError('no fold-in instances and no initial rows: nothing says how many entities are new')
            new_rows_init = models._glorot_uniform((int(y.max()) + 1, np.shape(R_e)[1]))
        new_rows_init = np.ascontiguousarray(new_rows_init, dtype=np.float32)
        if seed is None:
            seed = int(np.random.randint(low=0, high=(1 << 30)))
        self.window_size = int(window_size)
        self.num_new = int(new_rows_init.shape[0])
        self.refresh = None if refresh is None else refresh.copy()
        self.num_refresh = 0 if refresh is None else int(refresh.size)
        self.num_entities = int(np.shape(R_e)[0])
        self.training_num_instances = int(y.shape[0])
        _capi.require_gpu()
        self._attach(_engine, lambda: self._vs_engine(R_w, R_e, W, b, self.window_size, device),
                     lambda engine: _capi.FoldIn(engine, new_rows_init, batch_size, num_negative_samples, regularization_lambda,
                                                 lr=lr, seed=seed, refresh_ids=refresh))
        self._foldin.upload(x, y, w)
        if refresh is None:
            logging.info('Folding in %d new entities (rows %d .. %d) on %d instances.', self.num_new, self.num_entities,
                         self.num_entities + self.num_new - 1, self.training_num_instances)
        else:
            logging.info('Refreshing %d trained entities and folding in %d new ones on %d instances.', self.num_refresh,
                         self.num_new, self.training_num_instances)

    @classmethod
    def from_model(cls, model, new_rows_init, training_set, batch_size, num_negative_samples, regularization_lambda,
                   seed=None, lr=1e-3, refresh=None):
        """From a live ``models.VectorSpaceLanguageModel``: its parameters as they are now are copied on the device (the
        model may train on or be dropped afterwards)."""
        if not isinstance(model, models.VectorSpaceLanguageModel):
            raise RuntimeError('a fold-in needs a VectorSpaceLanguageModel')
        shape = (model.num_entities, model.entity_representation_size)
        return cls(None, _Shape(shape), None, None, new_rows_init, training_set, batch_size, num_negative_samples,
                   regularization_lambda, model.window_size, seed=seed, lr=lr, _engine=model._engine, refresh=refresh)

    # -- results and state --------------------------------------------------------------------------------------------
    def get_new_representations(self):
        """(N, d_e): the new rows as they are now."""
        return self._foldin.get_rows(_capi.FOLDIN_ROWS)[self.num_refresh:]

    def get_refreshed_representations(self):
        """(len(refresh), d_e): the refreshed trained rows as they are now, in the order of ``refresh``."""
        return self._foldin.get_rows(_capi.FOLDIN_ROWS)[:self.num_refresh]

    def get_extended_representations(self, R_e):
        """(V_e + N, d_e): the trained rows ``R_e`` (the caller's: never modified) with the rows of ``refresh`` replaced by
        their slots and the new rows behind."""
        R_e = np.asarray(R_e, dtype=np.float32)
        assert R_e.shape[0] == self.num_entities
        rows = self._foldin.get_rows(_capi.FOLDIN_ROWS)
        ext = np.concatenate([R_e, rows[self.num_refresh:]], axis=0)
        if self.num_refresh:
            ext[self.refresh] = rows[:self.num_refresh]
        return ext


class _LlFoldInModel(_FoldInModel):
    """The two fold-ins of a loglinear model on top of it: the throwaway engine and the labels of either form."""

    @staticmethod
    def _ll_engine(R_w, W, b, window_size, device):
        """A parameters-only loglinear model on the device that holds the frozen tensors."""
        Rw, Wt, bt = (np.asarray(a, dtype=np.float32) for a in (R_w, W, b))
        assert Wt.shape[0] == Rw.shape[1] and bt.shape == (Wt.shape[1],)
        engine = _capi.Engine(
            kind=_capi.KIND_LOGLINEAR, batch_size=1, global_batch_size=1, window_size=window_size,
            vocab_size=Rw.shape[0], num_entities=Wt.shape[1], word_dim=Rw.shape[1], entity_dim=0, num_negatives=0,
            id_bytes=4, device=device, keep_grads=0, deterministic=1, inference_only=1, lambda_=0.0, lr=1.0, beta1=0.95,
            beta2=0.0, eps=1e-6, seed=0)
        for which, value in ((_capi.T_RW, Rw), (_capi.T_W, Wt), (_capi.T_B, bt)):
            engine.set_tensor(which, value)
        return engine

    @staticmethod
    def _labels(x, y, window_size):
        """-> (y, rows).  rows: y is a ``scipy.sparse`` matrix of label rows, returned as canonical CSR (a copy: the caller's
        matrix is not modified); otherwise y is returned as the (M,) array of one label per instance."""
        rows = scipy.sparse.issparse(y)
        if rows:
            y = scipy.sparse.csr_matrix(y, dtype=np.float32, copy=True)
            y.sum_duplicates()
            y.sort_indices()
            assert x.ndim == 2 and x.shape[1] == window_size and y.shape[0] == x.shape[0]
        else:
            y = np.asarray(y)
            assert x.ndim == 2 and x.shape[1] == window_size and y.ndim == 1 and y.shape[0] == x.shape[0]
        return y, rows

    def _upload(self, x, y, w, rows):
        if rows:
            self._foldin.upload_csr(x, y.indptr, y.indices, y.data, w)
        else:
            self._foldin.upload(x, y, w)


class LogLinearFoldIn(_LlFoldInModel):
    """N new entities learnt on top of a trained loglinear model (R_w, W (d, V_e), b (V_e): host arrays, never written):
    N new columns Wn (d, N) of the output layer and N new biases bn, with the model's own loss over the V_e + N entities
    (include/sert_hip_ll_foldin.h).

    training_set: (x (M, window_size) token ids of the TRAINED vocabulary, y (M,) in [0, N), w (M,) weights or None).
    New entity e becomes column V_e + e.  ``new_W_init`` None: N = y.max() + 1 columns drawn with
    ``_glorot_uniform((d, N))``; ``new_b_init`` None: zeros -- as models.LanguageModel initialises its output layer.  The
    batch size and lambda are the fold-in's own.  ``max_cache_bytes``: a cap on the logit cache of the upload (0: none).

    Label rows: y may be a ``scipy.sparse`` matrix (M, V_e + N) instead -- the label DISTRIBUTIONS the model was trained on
    without --one_hot_classes.  Column e < V_e is trained entity e: a label only (a co-author the model knows), its column of
    W stays frozen; column V_e + j is new entity j.  The matrix is brought to canonical CSR (``tocsr``, ``sum_duplicates``,
    ``sort_indices``); with ``new_W_init`` None, N = y.shape[1] - V_e, which must be at least 1.

    ``refresh`` (an array of distinct trained internal indices): these trained columns and biases learn too -- people the
    model knows who wrote new documents.  The trainable columns are then SLOTS, the refreshed columns first, in the order of
    ``refresh``, the new columns behind them: an integer y is a slot in [0, len(refresh) + N), and ``new_W_init`` may be None
    or empty (nothing is new; with label rows None still means N = y.shape[1] - V_e, which may then be 0).  Label rows keep
    their columns: a trained column that is refreshed is a parameter, one that is not stays a frozen co-label.  A refreshed
    column starts from its trained value and bias and learns from the instances given: to keep its old evidence, pass the
    entity's old documents along with the new ones."""

    def __init__(self, R_w, W, b, new_W_init, new_b_init, training_set, batch_size, regularization_lambda, window_size,
                 device=0, max_cache_bytes=0, _engine=None, refresh=None):
        super(LogLinearFoldIn, self).__init__(batch_size)
        if refresh is not None:
            refresh = np.asarray(refresh, dtype=np.int64).reshape(-1)
        x = np.asarray(training_set[0])
        w = training_set[2] if len(training_set) > 2 else None
        word_dim, num_entities = int(np.shape(W)[0]), int(np.shape(W)[1])
        y, rows = self._labels(x, training_set[1], window_size)     # (label rows: over the V_e + N columns)
        if rows:
            if new_W_init is None:
                if y.shape[1] - num_entities < (1 if refresh is None else 0):
                    raise RuntimeError('label rows of %d columns on a model of %d entities: no column is new'
                                       % (y.shape[1], num_entities))
                new_W_init = (models._glorot_uniform((word_dim, y.shape[1] - num_entities)) if y.shape[1] > num_entities
                              else np.zeros((word_dim, 0), dtype=np.float32))
        else:
            if new_W_init is None and refresh is not None:
                new_W_init = np.zeros((word_dim, 0), dtype=np.float32)
            if new_W_init is None:
                if not y.size:
                    raise RuntimeError('no fold-in instances and no initial columns: nothing says how many entities are new')
                new_W_init = models._glorot_uniform((word_dim, int(y.max()) + 1))
        new_W_init = np.ascontiguousarray(new_W_init, dtype=np.float32).reshape(word_dim, -1)
        if rows and y.shape[1] != num_entities + new_W_init.shape[1]:
            raise RuntimeError('label rows must have V_e + N = %d + %d columns, not %d'
                               % (num_entities, new_W_init.shape[1], y.shape[1]))
        self.window_size = int(window_size)
        self.num_new = int(new_W_init.shape[1])
        self.refresh = None if refresh is None else refresh.copy()
        self.num_refresh = 0 if refresh is None else int(refresh.size)
        self.num_entities = int(np.shape(W)[1])
        self.training_num_instances = int(y.shape[0])
        _capi.require_gpu()
        self._attach(_engine, lambda: self._ll_engine(R_w, W, b, self.window_size, device),
                     lambda engine: _capi.LlFoldIn(engine, new_W_init, new_b_init, batch_size, regularization_lambda,
                                                   max_cache_bytes=max_cache_bytes, refresh_ids=refresh))
        self._upload(x, y, w, rows)
        if refresh is None:
            logging.info('Folding in %d new entities (columns %d .. %d) on %d instances%s.', self.num_new, self.num_entities,
                         self.num_entities + self.num_new - 1, self.training_num_instances,
                         ' with %d label entries' % y.nnz if rows else '')
        else:
            logging.info('Refreshing %d trained entities and folding in %d new ones on %d instances%s.', self.num_refresh,
                         self.num_new, self.training_num_instances, ' with %d label entries' % y.nnz if rows else '')

    @classmethod
    def from_model(cls, model, new_W_init, new_b_init, training_set, batch_size, regularization_lambda, max_cache_bytes=0,
                   refresh=None):
        """From a live ``models.LanguageModel``: its parameters as they are now are copied on the device (the model may train
        on or be dropped afterwards)."""
        if not isinstance(model, models.LanguageModel):
            raise RuntimeError('a loglinear fold-in needs a LanguageModel')
        return cls(None, _Shape((model.representation_size, model.output_layer_size)), None, new_W_init, new_b_init,
                   training_set, batch_size, regularization_lambda, model.window_size, max_cache_bytes=max_cache_bytes,
                   _engine=model._engine, refresh=refresh)

    # -- results and state --------------------------------------------------------------------------------------------
    def get_new_dense(self):
        """(Wn (d, N), bn (N,)): the new columns and biases as they are now."""
        R = self.num_refresh
        return (np.ascontiguousarray(self._foldin.get_tensor(_capi.LL_FOLDIN_W)[:, R:]),
                np.ascontiguousarray(self._foldin.get_tensor(_capi.LL_FOLDIN_B)[R:]))

    def get_refreshed_dense(self):
        """(W (d, len(refresh)), b (len(refresh),)): the refreshed trained columns and biases as they are now, in the order of
        ``refresh``."""
        R = self.num_refresh
        return (np.ascontiguousarray(self._foldin.get_tensor(_capi.LL_FOLDIN_W)[:, :R]),
                np.ascontiguousarray(self._foldin.get_tensor(_capi.LL_FOLDIN_B)[:R]))

    def get_extended_dense(self, W, b):
        """(W (d, V_e + N), b (V_e + N,)): the trained ``W`` / ``b`` (the caller's: never modified) with the columns of
        ``refresh`` replaced by their slots and the new columns behind."""
        W, b = np.asarray(W, dtype=np.float32), np.asarray(b, dtype=np.float32)
        assert W.shape[1] == self.num_entities and b.shape == (self.num_entities,)
        Wt, bt = self._foldin.get_tensor(_capi.LL_FOLDIN_W), self._foldin.get_tensor(_capi.LL_FOLDIN_B)
        R = self.num_refresh
        Wx, bx = np.concatenate([W, Wt[:, R:]], axis=1), np.concatenate([b, bt[R:]])
        if R:
            Wx[:, self.refresh] = Wt[:, :R]
            bx[self.refresh] = bt[:R]
        return Wx, bx

    def get_optimizer_state(self):
        g = self._foldin.get_tensor
        return {'accu_W': g(_capi.LL_FOLDIN_ACCU_W), 'accu_b': g(_capi.LL_FOLDIN_ACCU_B),
                'delta_W': g(_capi.LL_FOLDIN_DELTA_W), 'delta_b': g(_capi.LL_FOLDIN_DELTA_B)}

    def set_optimizer_state(self, st):
        for name, which in (('accu_W', _capi.LL_FOLDIN_ACCU_W), ('accu_b', _capi.LL_FOLDIN_ACCU_B),
                            ('delta_W', _capi.LL_FOLDIN_DELTA_W), ('delta_b', _capi.LL_FOLDIN_DELTA_B)):
            self._foldin.set_tensor(which, st[name])


def new_word_rows(vocab_size, num_new_words, word_dim):
    """(Nw, d_w) initial rows from the global np.random, uniform within the bound bin/train.py drew the trained R_w in:
    Glorot's sqrt(6 / (V_w + d_w)), the fan of the trained table.  (Glorot on the (Nw, d_w) block alone would make a handful
    of new rows several times larger than every trained one.)"""
    a = np.sqrt(6.0 / (vocab_size + word_dim))
    return np.random.uniform(low=-a, high=a, size=(num_new_words, word_dim)).astype(np.float32)


def _word_rows_init(new_rows_init, x, table_shape):
    """The initial rows of a word fold-in as a float32 array; None: as many rows as x names new words, drawn by
    ``new_word_rows``.  table_shape: (V_w, d) of the trained word table."""
    vocab_size, word_dim = int(table_shape[0]), int(table_shape[1])
    if new_rows_init is None:
        if not x.size or int(x.max()) < vocab_size:
            raise RuntimeError('no token of a new word and no initial rows: nothing says how many words are new')
        new_rows_init = new_word_rows(vocab_size, int(x.max()) + 1 - vocab_size, word_dim)
    return np.ascontiguousarray(new_rows_init, dtype=np.float32)


class WordFoldIn(_NceFoldInModel):
    """Nw new word rows learnt on top of a trained vectorspace model (R_w, R_e, W, b: host arrays, never written).

    training_set: (x (M, window_size) token ids in [0, V_w + Nw) -- new word v is id V_w + v --, y (M,) trained entity
    indices in [0, V_e), w (M,) weights or None).  ``new_rows_init`` None: Nw = x.max() + 1 - V_w rows drawn by
    ``new_word_rows``, at the scale bin/train.py drew the trained rows.  The batch size, the number of negatives, lambda and the
    learning rate are the fold-in's own.  An instance without a new word is legal: it adds to the loss and moves nothing."""

    #: negative_sampler / eval_negative_sampler draw from [0, V_e)
    _moment_keys = ('m_Nv', 'v_Nv')

    def __init__(self, R_w, R_e, W, b, new_rows_init, training_set, batch_size, num_negative_samples,
                 regularization_lambda, window_size, seed=None, lr=1e-3, device=0, _engine=None):
        super(WordFoldIn, self).__init__(batch_size)
        x, y = np.asarray(training_set[0]), np.asarray(training_set[1])
        w = training_set[2] if len(training_set) > 2 else None
        assert x.ndim == 2 and x.shape[1] == window_size and y.ndim == 1 and y.shape[0] == x.shape[0]
        vocab_size = int(np.shape(R_w)[0])
        new_rows_init = _word_rows_init(new_rows_init, x, np.shape(R_w))
        if seed is None:
            seed = int(np.random.randint(low=0, high=(1 << 30)))
        self.window_size = int(window_size)
        self.num_new_words = int(new_rows_init.shape[0])
        self.vocab_size = vocab_size
        self.training_num_instances = int(y.shape[0])
        _capi.require_gpu()
        self._attach(_engine, lambda: self._vs_engine(R_w, R_e, W, b, self.window_size, device),
                     lambda engine: _capi.WordFoldIn(engine, new_rows_init, batch_size, num_negative_samples,
                                                     regularization_lambda, lr=lr, seed=seed))
        self._foldin.upload(x, y, w)
        logging.info('Folding in %d new words (token ids %d .. %d) on %d instances.', self.num_new_words, vocab_size,
                     vocab_size + self.num_new_words - 1, self.training_num_instances)

    @classmethod
    def from_model(cls, model, new_rows_init, training_set, batch_size, num_negative_samples, regularization_lambda,
                   seed=None, lr=1e-3):
        """From a live ``models.VectorSpaceLanguageModel``: its parameters as they are now are copied on the device (the
        model may train on or be dropped afterwards)."""
        if not isinstance(model, models.VectorSpaceLanguageModel):
            raise RuntimeError('a word fold-in needs a VectorSpaceLanguageModel')
        cfg = model._engine.cfg
        return cls(_Shape((int(cfg.vocab_size), int(cfg.word_dim))), None, None, None, new_rows_init, training_set, batch_size,
                   num_negative_samples, regularization_lambda, model.window_size, seed=seed, lr=lr, _engine=model._engine)

    # -- results and state --------------------------------------------------------------------------------------------
    def get_new_word_representations(self):
        """(Nw, d_w): the new rows as they are now."""
        return self._foldin.get_rows(_capi.WFOLD_ROWS)

    def get_extended_word_representations(self, R_w):
        """(V_w + Nw, d_w): the trained rows ``R_w`` (the caller's: never modified) with the new rows behind."""
        R_w = np.asarray(R_w, dtype=np.float32)
        assert R_w.shape[0] == self.vocab_size
        return np.concatenate([R_w, self._foldin.get_rows(_capi.WFOLD_ROWS)], axis=0)


class LogLinearWordFoldIn(_LlFoldInModel):
    """Nw new word rows learnt on top of a trained loglinear model (R_w, W (d, V_e), b (V_e): host arrays, never written), with
    the model's own loss (include/sert_hip_ll_wfold.h).

    training_set: (x (M, window_size) token ids in [0, V_w + Nw) -- new word v is id V_w + v --, y (M,) trained entity
    indices in [0, V_e), w (M,) weights or None).  ``new_rows_init`` None: Nw = x.max() + 1 - V_w rows drawn by
    ``new_word_rows``, at the scale bin/train.py drew the trained rows.  The batch size and lambda are the fold-in's own.
    ``max_cache_bytes``: a cap on the frozen table of the upload (0: none).  An instance without a new word is legal: it adds to
    the loss and moves nothing.

    Label rows: y may be a ``scipy.sparse`` matrix (M, V_e) instead -- the label DISTRIBUTIONS the model was trained on
    without --one_hot_classes, over the trained entities (a word fold-in has no new column).  The matrix is brought to
    canonical CSR (``tocsr``, ``sum_duplicates``, ``sort_indices``) and uploaded as rows: the new word rows are then fitted
    with the loss that produced the frozen parameters beside them."""

    def __init__(self, R_w, W, b, new_rows_init, training_set, batch_size, regularization_lambda, window_size, device=0,
                 max_cache_bytes=0, _engine=None):
        super(LogLinearWordFoldIn, self).__init__(batch_size)
        x = np.asarray(training_set[0])
        w = training_set[2] if len(training_set) > 2 else None
        y, rows = self._labels(x, training_set[1], window_size)     # (label rows: over the V_e trained columns)
        vocab_size = int(np.shape(R_w)[0])
        new_rows_init = _word_rows_init(new_rows_init, x, np.shape(R_w))
        self.window_size = int(window_size)
        self.num_new_words = int(new_rows_init.shape[0])
        self.vocab_size = vocab_size
        self.training_num_instances = int(y.shape[0])
        _capi.require_gpu()
        self._attach(_engine, lambda: self._ll_engine(R_w, W, b, self.window_size, device),
                     lambda engine: _capi.LlWordFoldIn(engine, new_rows_init, batch_size, regularization_lambda,
                                                       max_cache_bytes=max_cache_bytes))
        if rows and y.shape[1] != self._foldin.num_entities:
            raise RuntimeError('label rows must have V_e = %d columns, not %d: a word fold-in has no new entity'
                               % (self._foldin.num_entities, y.shape[1]))
        self._upload(x, y, w, rows)
        logging.info('Folding in %d new words (token ids %d .. %d) on %d instances%s.', self.num_new_words, vocab_size,
                     vocab_size + self.num_new_words - 1, self.training_num_instances,
                     ' with %d label entries' % y.nnz if rows else '')

    @classmethod
    def from_model(cls, model, new_rows_init, training_set, batch_size, regularization_lambda, max_cache_bytes=0):
        """From a live ``models.LanguageModel``: its parameters as they are now are copied on the device (the model may train
        on or be dropped afterwards)."""
        if not isinstance(model, models.LanguageModel):
            raise RuntimeError('a loglinear word fold-in needs a LanguageModel')
        cfg = model._engine.cfg
        return cls(_Shape((int(cfg.vocab_size), int(cfg.word_dim))), None, None, new_rows_init, training_set, batch_size,
                   regularization_lambda, model.window_size, max_cache_bytes=max_cache_bytes, _engine=model._engine)

    # -- results and state --------------------------------------------------------------------------------------------
    def get_new_word_representations(self):
        """(Nw, d): the new rows as they are now."""
        return self._foldin.get_rows(_capi.LL_WFOLD_ROWS)

    def get_extended_word_representations(self, R_w):
        """(V_w + Nw, d): the trained rows ``R_w`` (the caller's: never modified) with the new rows behind."""
        R_w = np.asarray(R_w, dtype=np.float32)
        assert R_w.shape[0] == self.vocab_size
        return np.concatenate([R_w, self._foldin.get_rows(_capi.LL_WFOLD_ROWS)], axis=0)

    def get_optimizer_state(self):
        return {'accu_Nv': self._foldin.get_rows(_capi.LL_WFOLD_ACCU), 'delta_Nv': self._foldin.get_rows(_capi.LL_WFOLD_DELTA)}

    def set_optimizer_state(self, st):
        self._foldin.set_rows(_capi.LL_WFOLD_ACCU, st['accu_Nv'])
        self._foldin.set_rows(_capi.LL_WFOLD_DELTA, st['delta_Nv'])


class _Shape(object):
    """Stands in for a table the constructor only asks the shape of (from_model: the table itself stays on the device)."""

    def __init__(self, shape):
        self.shape = shape


# ---- the model dump and the meta of the extended model (bin/fold_in.py) -------------------------------------------------

def extend_dump(args, predict_fn, R_w, R_e, new_rows):
    """The objects of a model dump (training.EpochDriver.dump: args, predict_fn, R_w, R_e) with R_e extended by the new rows."""
    R_e = np.asarray(R_e)
    new_rows = np.asarray(new_rows, dtype=R_e.dtype)
    assert new_rows.ndim == 2 and new_rows.shape[1] == R_e.shape[1]
    return [args, predict_fn, R_w, np.concatenate([R_e, new_rows], axis=0)]


def extend_ll_dump(args, predict_fn, R_w, Wn, bn):
    """The objects of a loglinear model dump (args, predict_fn, R_w) whose LogLinearPredictFn holds W (d, V_e + N) and
    b (V_e + N): the trained output layer of ``predict_fn`` (never modified) with the new columns ``Wn`` (d, N) and biases
    ``bn`` (N) behind.  bin/query.py and LogLinearPredictFn.rank_queries serve it unchanged."""
    st = predict_fn.__getstate__()
    W, b = np.asarray(st['W']), np.asarray(st['b'])
    Wn, bn = np.asarray(Wn, dtype=W.dtype), np.asarray(bn, dtype=b.dtype)
    assert Wn.ndim == 2 and Wn.shape[0] == W.shape[0] and bn.shape == (Wn.shape[1],)
    extended = models.LogLinearPredictFn(R_w=np.asarray(st['R_w']), W=np.concatenate([W, Wn], axis=1),
                                         b=np.concatenate([b, bn]), window_size=st['window_size'])
    return [args, extended, R_w]


def refresh_ll_dump(args, predict_fn, R_w, refresh, Wr, br, Wn, bn):
    """extend_ll_dump with the columns ``refresh`` of the trained output layer replaced by ``Wr`` (d, len(refresh)) / ``br`` and
    the new columns ``Wn`` / ``bn`` appended; ``predict_fn`` is not modified, every other column keeps its bits."""
    st = predict_fn.__getstate__()
    W, b = np.array(st['W'], copy=True), np.array(st['b'], copy=True)
    refresh = np.asarray(refresh, dtype=np.int64).reshape(-1)
    Wr, br = np.asarray(Wr, dtype=W.dtype).reshape(W.shape[0], -1), np.asarray(br, dtype=b.dtype).reshape(-1)
    assert Wr.shape == (W.shape[0], refresh.size) and br.shape == (refresh.size,)
    W[:, refresh] = Wr
    b[refresh] = br
    replaced = models.LogLinearPredictFn(R_w=np.asarray(st['R_w']), W=W, b=b, window_size=st['window_size'])
    return extend_ll_dump(args, replaced, R_w, np.asarray(Wn, dtype=W.dtype).reshape(W.shape[0], -1), np.asarray(bn).reshape(-1))


def extend_words_dump(args, predict_fn, R_w, R_e, new_rows):
    """The objects of a model dump (args, predict_fn, R_w, R_e) with R_w extended by the rows of the new words; the caller's
    R_w is not modified, R_e and predict_fn (W, b) are the trained ones."""
    R_w = np.asarray(R_w)
    new_rows = np.asarray(new_rows, dtype=R_w.dtype)
    assert new_rows.ndim == 2 and new_rows.shape[1] == R_w.shape[1]
    return [args, predict_fn, np.concatenate([R_w, new_rows], axis=0), R_e]


def extend_ll_words_dump(args, predict_fn, R_w, new_rows):
    """The objects of a loglinear model dump (args, LogLinearPredictFn, R_w) with the word table extended by the rows of the
    new words, in the dump and in the predict function alike; the caller's R_w and ``predict_fn`` are not modified, W and b are
    the trained ones.  bin/query.py and LogLinearPredictFn.rank_queries serve it unchanged."""
    st = predict_fn.__getstate__()
    R_w = np.asarray(R_w)
    trained = np.asarray(st['R_w'])
    new_rows = np.asarray(new_rows, dtype=R_w.dtype)
    assert new_rows.ndim == 2 and new_rows.shape[1] == R_w.shape[1] and trained.shape == R_w.shape
    extended = models.LogLinearPredictFn(R_w=np.concatenate([trained, new_rows.astype(trained.dtype)], axis=0), W=np.asarray(st['W']),
                                         b=np.asarray(st['b']), window_size=st['window_size'])
    return [args, extended, np.concatenate([R_w, new_rows], axis=0)]


WORDS_FIRST_ADVICE = ('fold the entities in first (bin/fold_in.py without --new_words) and prepare the documents against the '
                      'extended meta (bin/prepare.py --vocabulary_from META_EXT --extend_vocabulary)')


def new_words_of(meta, new_meta):
    """The words ``new_meta`` appends to the vocabulary of ``meta``, in id order (ids V_w, V_w + 1, ...).  Refused: a
    ``new_meta`` whose vocabulary is not the trained one, every word at its trained id, with ids V_w .. appended
    (bin/prepare.py --vocabulary_from META --extend_vocabulary)."""
    words, tokens = meta[1], meta[2]
    new_words, new_tokens = new_meta[1], new_meta[2]
    V_w, V_x = len(words), len(new_words)
    ok = (V_x >= V_w and len(new_tokens) == V_x and sorted(new_tokens) == list(range(V_x)) and
          all(new_tokens[i] == tokens[i] for i in range(V_w)) and
          all(new_words[w].id == entry.id for w, entry in words.items() if w in new_words) and
          all(w in new_words for w in words) and all(new_words[new_tokens[i]].id == i for i in range(V_x)))
    if not ok:
        raise RuntimeError('the vocabulary of the new meta is not the trained one with new words appended behind it: prepare '
                           'the documents with --vocabulary_from META --extend_vocabulary')
    return [new_tokens[i] for i in range(V_w, V_x)]


def extend_meta_words(meta, new_meta):
    """The five pickles of a meta file for a model whose VOCABULARY grew: ``words`` and ``tokens`` are ``new_meta``'s (the
    trained words at their trained ids, the new ones at V_w ..); the entity index is the trained one and the associations of
    ``new_meta`` are added to it (merge_meta's rule for known ids).  Refused: a vocabulary that does not extend the trained
    one (new_words_of), and an entity of ``new_meta`` that ``meta`` does not know."""
    new_words_of(meta, new_meta)
    new_index = new_meta[3]
    entity_ids = [new_index[e] for e in range(len(new_index))]
    known = set(meta[3].values())
    unknown = [e for e in entity_ids if e not in known]
    if unknown:
        raise RuntimeError('entity ids the trained model does not know: %r; %s' % (unknown[:5], WORDS_FIRST_ADVICE))
    associations = dict((e, new_meta[4].get(e, [])) for e in entity_ids)
    merged, _, new_ids, _ = merge_meta(meta, entity_ids, associations)
    assert not new_ids
    return [merged[0], new_meta[1], new_meta[2], merged[3], merged[4]]


def write_dump(path, objects):
    with open(path, 'wb') as f:
        for obj in objects:
            pickle.dump(obj, f, protocol=pickle.HIGHEST_PROTOCOL)


def extend_meta(meta, new_entity_ids, new_associations=None):
    """The five pickles of a meta file (args, words, tokens, entity_indices_inv, documents_per_entity) for the extended
    model: ``new_entity_ids[e]`` gets internal index V_e + e, ``new_associations`` (entity id -> document ids) are added.
    An id the meta already knows is refused; ``words`` / ``tokens`` are the trained model's, untouched."""
    args, words, tokens, entity_indices_inv, assocs = meta
    new_entity_ids = list(new_entity_ids)
    known = set(entity_indices_inv.values())
    clash = [e for e in new_entity_ids if e in known]
    if clash:
        raise RuntimeError('entity ids already in the trained model: %r' % (clash[:5],))
    if len(set(new_entity_ids)) != len(new_entity_ids):
        raise RuntimeError('duplicate new entity ids')
    V_e = len(entity_indices_inv)
    assert sorted(entity_indices_inv) == list(range(V_e)), 'internal entity indices must be 0 .. V_e - 1'
    extended = dict(entity_indices_inv)
    for e, entity_id in enumerate(new_entity_ids):
        extended[V_e + e] = entity_id
    merged = dict(assocs)
    for entity_id, documents in (new_associations or {}).items():
        merged[entity_id] = list(merged.get(entity_id, [])) + list(documents)
    return [args, words, tokens, extended, merged]


def merge_meta(meta, entity_ids, associations=None):
    """The meta of a model in which entities GAIN documents (bin/fold_in.py --refresh; --unfreeze_known for a loglinear dump).  ``entity_ids[k]`` is entity k of the
    new documents' meta: an id the trained meta knows keeps its internal index and is refreshed, an unknown one gets
    V_e + e in order of first appearance; ``associations`` (entity id -> document ids) are added to either kind.
    -> (the five pickles, the refreshed internal indices in order of first appearance, the new ids, slots): ``slots[k]`` is
    the slot of entity k in a fold-in with ``refresh`` = the refreshed indices -- refreshed slots first, new ones behind."""
    args, words, tokens, entity_indices_inv, assocs = meta
    entity_ids = list(entity_ids)
    if len(set(entity_ids)) != len(entity_ids):
        raise RuntimeError('duplicate entity ids')
    V_e = len(entity_indices_inv)
    assert sorted(entity_indices_inv) == list(range(V_e)), 'internal entity indices must be 0 .. V_e - 1'
    index_of = dict((entity_id, index) for index, entity_id in entity_indices_inv.items())
    refreshed = [index_of[e] for e in entity_ids if e in index_of]
    new_ids = [e for e in entity_ids if e not in index_of]
    extended = dict(entity_indices_inv)
    for e, entity_id in enumerate(new_ids):
        extended[V_e + e] = entity_id
    slot_of_index = dict((index, s) for s, index in enumerate(refreshed))
    slot_of_new = dict((entity_id, len(refreshed) + e) for e, entity_id in enumerate(new_ids))
    slots = np.array([slot_of_index[index_of[e]] if e in index_of else slot_of_new[e] for e in entity_ids], dtype=np.int32)
    merged = dict(assocs)
    for entity_id, documents in (associations or {}).items():
        merged[entity_id] = list(merged.get(entity_id, [])) + list(documents)
    return [args, words, tokens, extended, merged], np.array(refreshed, dtype=np.int32), new_ids, slots


def label_columns(meta, entity_ids, associations=None):
    """The columns of label rows over the entities of a new documents' meta (bin/fold_in.py --label_distributions).
    ``entity_ids[k]`` is entity k of that meta: an id the trained meta knows maps to its trained internal index -- a frozen
    co-label --, an unknown one to V_e + its position among the unknown ones.  ``associations`` (entity id -> document
    ids) are added to either kind.  -> (the five pickles of the merged meta, columns (len(entity_ids),) int32, the new ids
    in column order).  All of it is merge_meta's: a known id is what it calls refreshed."""
    merged, known, new_ids, slots = merge_meta(meta, entity_ids, associations)
    V_e = len(meta[3])
    columns = np.concatenate([known, V_e + np.arange(len(new_ids), dtype=np.int32)]).astype(np.int32)[slots]
    return merged, columns.reshape(-1), new_ids


def remap_label_columns(y, columns, num_columns):
    """The sparse label matrix ``y`` (M, len(columns)) with column k moved to ``columns[k]`` of ``num_columns``: canonical CSR."""
    y = scipy.sparse.coo_matrix(y)
    columns = np.asarray(columns, dtype=np.int64)
    assert y.shape[1] <= columns.size and (columns.size == 0 or columns.max() < num_columns)
    out = scipy.sparse.csr_matrix((y.data.astype(np.float32), (y.row, columns[y.col])), shape=(y.shape[0], num_columns))
    out.sum_duplicates()
    out.sort_indices()
    return out


def refresh_dump(args, predict_fn, R_w, R_e, refresh, refreshed_rows, new_rows):
    """The objects of a model dump with the rows ``refresh`` of R_e replaced by ``refreshed_rows`` and ``new_rows`` appended;
    the caller's R_e is not modified."""
    R_e = np.array(R_e, copy=True)
    refresh = np.asarray(refresh, dtype=np.int64)
    refreshed_rows = np.asarray(refreshed_rows, dtype=R_e.dtype)
    assert refreshed_rows.shape == (refresh.size, R_e.shape[1])
    R_e[refresh] = refreshed_rows
    return extend_dump(args, predict_fn, R_w, R_e, np.asarray(new_rows, dtype=R_e.dtype).reshape(-1, R_e.shape[1]))


def read_meta(path):
    with open(path, 'rb') as f:
        return [pickle.load(f) for _ in range(5)]


def write_meta(path, meta):
    with open(path, 'wb') as f:
        for obj in meta:
            pickle.dump(obj, f, protocol=pickle.HIGHEST_PROTOCOL)
