"""The miswordpolyenc scoring route: WordSentAlignPolyEnc and the TrainedScoringModel that pp_gen_nearest.py ranks pools with.

Drop-in for the test-time surface of WordSentAlignPolyEnc (src/learning/facetid_models/disent_models.py:840-925: ``score``) and
TrainedScoringModel (src/pre_process/pp_gen_nearest.py:36-87: ``predict``), plus the ranking its callers write
(pp_gen_nearest.py:436-456):

    model = TrainedScoringModel('miswordpolyenc', trained_model_path)      # run_info.json + model_cur_best.pt
    ret = model.predict(query=query_sent_reps, cands=pool_sent_reps)       # {'cand_scores': [...], 'pair_scores': [[ql, cl], ...]}
    ranked = model.rank(query_sent_reps, pool_sent_reps, cand_pids)        # [(pid, -sim), ...] best first

The encoder is AspireConSent's (the reference class inherits WordSentAlignBiEnc's partial_forward / sent_reps_bert unchanged); the
score is aspire_jointsm_scores_f32 (include/aspire_hip.h, A14).  The model's dist_function,
pair_distances.allpair_joint_sm_negscore, is differentiable with respect to the sentence reps (aspire_jointsm_backward_f32), so its
triplet loss can be written; forward_rank and a trainer are still not built.
"""
import os

import numpy as np
import torch

from . import _lib, ops
from .consent import AspireConSent
from .model_front import read_hparams, strip_prefix


class WordSentAlignPolyEnc(AspireConSent):
    def __init__(self, model_hparams=None, bert_config=None, bert_model=None, matmul='fp32'):
        """
        :param model_hparams: the run's hyper-parameters (run_info.json 'all_hparams'): 'base-pt-layer' names the HF model to
            load; 'score_aggregation', when given, must be 'jointsm' (disent_models.py:868-871).
        :param bert_config: accepted for the reference's signature, not used.
        :param bert_model: an already constructed transformers BertModel instead of loading 'base-pt-layer'.
        """
        model_hparams = model_hparams or {}
        agg = model_hparams.get('score_aggregation', 'jointsm')
        if agg != 'jointsm':
            raise ValueError(f'Unknown aggregation: {agg}')
        AspireConSent.__init__(self, hf_model_name=model_hparams.get('base-pt-layer'), bert_model=bert_model, matmul=matmul)

    def load_state_dict(self, sd):
        """model_cur_best.pt: the encoder is rebuilt from its bert_encoder.* keys (the class has no other parameters)."""
        enc, _ = strip_prefix(sd, 'bert_encoder.', who='WordSentAlignPolyEnc')
        self._rebuild_encoder(enc)
        return self

    @staticmethod
    def score(query_reps, cand_reps):
        """disent_models.py:877-925.  query_reps: np [num_sents, 768]; cand_reps: list of np [num_sents, 768].  The reference pads
        the candidates, repeats the query per candidate and un-pads the soft-max again; here the un-padded documents go to the
        kernel as they are (one query against every candidate) and only pair_softmax travels in padded form.
        :return: {'batch_scores': np float32 [batch_size] similarities, 'pair_scores': list of np [ql, cl] joint soft-maxes}"""
        query_reps = np.asarray(query_reps, dtype=np.float32)
        cand_reps = [np.asarray(r, dtype=np.float32) for r in cand_reps]
        if not cand_reps:
            raise ValueError('max() arg is an empty sequence')          # cmax_sents = max(cand_lens), disent_models.py:889
        cand_lens = [r.shape[0] for r in cand_reps]
        qlen, cmax = query_reps.shape[0], max(cand_lens)
        dev = ops.require_gpu()
        padded = torch.zeros(len(cand_reps), cmax, query_reps.shape[1], device=dev)
        for bi, r in enumerate(cand_reps):
            padded[bi, :cand_lens[bi]] = torch.from_numpy(r)
        q = ops.DeviceRepSet.from_padded(torch.from_numpy(query_reps)[None], [qlen])
        c = ops.DeviceRepSet.from_padded(padded, cand_lens)
        sims, soft = ops.jointsm_scores(q, c, pairing=_lib.PAIR_CROSS, want_pair_softmax=True)
        soft = soft.cpu().numpy()
        return {'batch_scores': sims.cpu().numpy(), 'pair_scores': [soft[i, :qlen, :clen] for i, clen in enumerate(cand_lens)]}


class TrainedScoringModel:
    """pp_gen_nearest.py:36-87: the trained model behind scoringmodel_rank_pool_sentfaceted (:366-466) and its siblings."""

    def __init__(self, model_name, trained_model_path=None, model_version='cur_best', model=None):
        """model: an already built WordSentAlignPolyEnc (or nothing at all when only predict / rank are used: they read no
        weights) instead of run_info.json + model_<version>.pt under trained_model_path."""
        if model_name not in {'miswordpolyenc'}:
            raise ValueError(f'Unknown model: {model_name}')
        if model is None and trained_model_path is not None:
            model = WordSentAlignPolyEnc(model_hparams=read_hparams(trained_model_path))
            model.load_state_dict(torch.load(os.path.join(trained_model_path, 'model_{:s}.pt'.format(model_version)), map_location='cpu'))
        self.model_name = model_name
        self.model = model

    def predict(self, query, cands):
        """:param query: np [num_sents, 768]; :param cands: list of np [num_sents, 768], the pool.
        :return: {'cand_scores': list of float, 'pair_scores': list of np [ql, cl]}.  The reference scores groups of 128 candidates
            (:68-85); a pair's score depends on its two documents only, so the whole pool goes through one call."""
        if not len(cands):
            return {'cand_scores': [], 'pair_scores': []}
        score_dict = WordSentAlignPolyEnc.score(query_reps=query, cand_reps=cands)
        return {'cand_scores': score_dict['batch_scores'].tolist(), 'pair_scores': score_dict['pair_scores']}

    def rank(self, query, cands, cand_pids):
        """The re-ranked pool as pp_gen_nearest.py:450-456 writes it: [(pid, -sim), ...], highest similarity first, ties in pool
        order (sorted(..., reverse=True) is stable).  A pid listed twice keeps its LAST score at its first position, as the
        reference's cand2sims dict does (:441-444)."""
        cand_scores = self.predict(query, cands)['cand_scores']
        assert len(cand_pids) == len(cand_scores)            # :439
        cand2sims = {}
        for cpid, sim in zip(cand_pids, cand_scores):
            cand2sims[cpid] = sim
        return [(cpid, -1 * sim) for cpid, sim in sorted(cand2sims.items(), key=lambda i: i[1], reverse=True)]
