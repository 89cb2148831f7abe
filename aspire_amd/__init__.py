"""aspire_amd -- MI355X-native implementation of Aspire's query-vs-candidate scoring path.

The arithmetic lives in libaspire_hip.so (hand-written HIP for gfx950, C ABI in include/aspire_hip.h);
this package is the host-side mirror of the reference's Python call surface
(examples/ex_aspire_consent.py, examples/ex_aspire_consent_multimatch.py).
"""
from . import _lib  # noqa: F401  (fails loudly when the HIP library has not been built)
from .batch_prep import prepare_abstracts, prepare_bert_sentences  # noqa: F401
from .pair_distances import (AllPairMaskedWasserstein, AllPairMaskedAttention, allpair_masked_dist_l2max,  # noqa: F401
                             allpair_masked_dist_l2topk, allpair_joint_sm_negscore, rep_len_tup)
from .rank_loss import RankLoss, SupAlignRankLoss, cross_doc_l1, sent_reps_from_hidden  # noqa: F401
from .train_encoder import HipBertTrainEncoder  # noqa: F401
from .packing import PackedRows, packed_rows  # noqa: F401
from .cls_train import BiEncTrain, ClsTripletLoss, IctEncTrain, IctLoss, SentEncTrain  # noqa: F401
from .optim import HipAdam, HipAdamW, HipAdagrad, clip_grad_norm_, grad_norm  # noqa: F401
from .trainer import RankTrainer  # noqa: F401
from .ddp import GradReducer, RankTrainerDDP, broadcast_parameters  # noqa: F401
from .batchers import JsonlRankBatches, rank_batch_sources, write_shuffled_copies  # noqa: F401
from .align import (align_cocited, alignment_encoder, context_set, random_neg_sampler,  # noqa: F401
                    write_aligned_examples)
from .consent import AspireConSent  # noqa: F401
from .contextner import AspireConSenContextual, AspireContextNER, AspireNER  # noqa: F401
from .polyenc import WordSentAlignPolyEnc, TrainedScoringModel  # noqa: F401
from .baselines import BertMLM, BertNER, SimCSE  # noqa: F401
from .sbert import SentenceModel  # noqa: F401
from .models import MODEL_TABLE, get_model  # noqa: F401
from .nearest import DenseReps, rank_pool, rank_pool_faceted, write_ranked  # noqa: F401
