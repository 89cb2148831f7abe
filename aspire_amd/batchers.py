"""The jsonl batcher of the sentence-alignment models -- ``AbsSentTokBatcher`` / ``AbsSentTokBatcherPreAlign``
(src/learning/batchers.py), i.e. 'miswordbienc', 'miswordpolyenc' and 'sbalisentbienc' -- over ``batch_prep.make_batch``, with the
shuffled per-epoch copies the reference's shell step makes and the two callables ``RankTrainer`` / ``RankTrainerDDP`` take:

    write_shuffled_copies(data_path, model_path, train_hparams, seed)                  # once per run (rank 0 under DDP, world=num_gpus)
    train_batches, dev_batches = rank_batch_sources(data_path, model_path, train_hparams, tokenizer)
    RankTrainer(encoder, model_hparams, train_hparams, model_path, train_batches, dev_batches).train()

The files are one json example per line: 'query' (TITLE, ABSTRACT), 'pos_context' and, in the dev file, 'neg_context', the contexts of
the pre-aligned model carrying 'cc_align' / 'abs_align' (aspire_amd.align.write_aligned_examples writes them).

The 'cospecter' / 'cosentbert' / 'ictsentbert' batchers (AbsTripleBatcher, SentTripleBatcher.make_batch, AbsSentBatcher) are not
here: their example formats differ, and callers of aspire_amd.cls_train bring their own batches.
"""
import codecs
import json
import math
import os
import random

from .batch_prep import make_batch


class JsonlRankBatches:
    """GenericBatcher / SentTripleBatcher.next_batch / raw_batch_from_file (batchers.py:18-165) over make_batch: iterating yields the
    ``batch_rank`` dicts of the first `num_examples` lines of `ex_fname`, `batch_size` at a time.
      num_batches   ceil(num_examples / batch_size), 1 when num_examples <= batch_size; the last batch has what is left
      feed          'query' always, 'pos_context' / 'neg_context' where the lines have them (only the dev file has negatives)
      align_type    'cc_align' or 'abs_align': which pre-computed alignment becomes pos_align_idxs / neg_align_idxs
    Lines beyond num_examples are not read.  A file with fewer lines raises ValueError (the reference dies in next()).  Every
    iteration opens the file anew, so the object can be iterated again and gives the same batches."""

    def __init__(self, ex_fname, num_examples, batch_size, tokenizer, align_type='cc_align'):
        if num_examples <= 0 or batch_size <= 0:
            raise ValueError(f'num_examples ({num_examples}) and batch_size ({batch_size}) must be positive')
        self.ex_fname, self.tokenizer, self.align_type = ex_fname, tokenizer, align_type
        self.full_len, self.batch_size = int(num_examples), int(batch_size)
        self.num_batches = int(math.ceil(float(self.full_len) / self.batch_size)) if self.full_len > self.batch_size else 1

    def __len__(self):
        return self.num_batches

    def raw_batches(self):
        """the raw feeds make_batch gets: {'query_texts', 'pos_texts'?, 'neg_texts'?} per batch"""
        with codecs.open(self.ex_fname, 'r', 'utf-8') as ex_file:
            read = 0
            for _ in range(self.num_batches):
                count = min(self.batch_size, self.full_len - read)
                queries, pos, neg = [], [], []
                for _ in range(count):
                    line = ex_file.readline()
                    if not line.strip():
                        raise ValueError(f'{self.ex_fname} has {read} examples, num_examples asks for {self.full_len}')
                    ex = json.loads(line)
                    queries.append(ex['query'])
                    # both contexts are optional per line: encoding-only files carry neither, training files no negative
                    if 'pos_context' in ex:
                        pos.append(ex['pos_context'])
                    if 'neg_context' in ex:
                        neg.append(ex['neg_context'])
                    read += 1
                if neg and pos:
                    yield {'query_texts': queries, 'pos_texts': pos, 'neg_texts': neg}
                elif pos:
                    yield {'query_texts': queries, 'pos_texts': pos}
                else:
                    yield {'query_texts': queries}

    def __iter__(self):
        for feed in self.raw_batches():
            yield make_batch(feed, self.tokenizer, align_type=self.align_type)


def _basenames(train_hparams):
    """(train_basename, dev_basename): trainer.py:438-444"""
    suffix = train_hparams.get('train_suffix')
    return (f'train-{suffix}', f'dev-{suffix}') if suffix else ('train', 'dev')


def shuffled_fname(model_path, train_hparams, epoch, rank=None):
    """{model_path}/shuffled_data/{train_basename}-{epoch}.jsonl, or {train_basename}-{rank}-{epoch}.jsonl for a rank's shard"""
    base = _basenames(train_hparams)[0]
    name = f'{base}-{epoch}.jsonl' if rank is None else f'{base}-{rank}-{epoch}.jsonl'
    return os.path.join(model_path, 'shuffled_data', name)


def write_shuffled_copies(data_path, model_path, train_hparams, seed, world=1):
    """What the reference's shell step does with head, shuf and split (bin/learning/run_main_fsim.sh, run_main_fsim-ddp.sh): the
    first train_size lines of {data_path}/{train_basename}.jsonl, shuffled once per epoch of num_epochs into
    {model_path}/shuffled_data/{train_basename}-{epoch}.jsonl; with world > 1 each epoch's shuffle is cut into the ranks' shards
    {train_basename}-{rank}-{epoch}.jsonl of exactly train_size // world lines, the remainder lines left out (trainer.py:768-770).
    Line-level (no json is parsed) and deterministic in `seed`: the same seed writes the same bytes, epochs differ.  The lines are
    held in memory: a training file too large for that is out of scope here (shuffle it outside, e.g. with shuf, under these names).
    Returns the file names written, [epoch] or [epoch][rank]."""
    base = _basenames(train_hparams)[0]
    train_size, num_epochs = int(train_hparams['train_size']), int(train_hparams['num_epochs'])
    src = os.path.join(data_path, base + '.jsonl')
    lines = []
    with codecs.open(src, 'r', 'utf-8') as fp:
        for line in fp:
            if len(lines) == train_size:
                break
            lines.append(line if line.endswith('\n') else line + '\n')
    if len(lines) < train_size:
        raise ValueError(f'{src} has {len(lines)} examples, train_size asks for {train_size}')
    os.makedirs(os.path.join(model_path, 'shuffled_data'), exist_ok=True)
    rng = random.Random(seed)
    written = []
    for epoch in range(num_epochs):
        order = list(range(train_size))
        rng.shuffle(order)
        if world <= 1:
            parts = [(shuffled_fname(model_path, train_hparams, epoch), order)]
        else:
            per = train_size // world
            parts = [(shuffled_fname(model_path, train_hparams, epoch, rank), order[rank * per:(rank + 1) * per]) for rank in range(world)]
        for fname, idxs in parts:
            with codecs.open(fname, 'w', 'utf-8') as out:
                out.writelines(lines[i] for i in idxs)
        written.append(parts[0][0] if world <= 1 else [f for f, _ in parts])
    return written


def rank_batch_sources(data_path, model_path, train_hparams, tokenizer, rank=None, world=1, align_type='cc_align'):
    """(train_batches, dev_batches), the callables RankTrainer / RankTrainerDDP take, over the files write_shuffled_copies wrote and
    {data_path}/{dev_basename}.jsonl (trainer.py:445-453).  train_batches(epoch) reads train_size examples (train_size // world of
    THIS rank's shard when rank is given and world > 1; with world <= 1 the un-sharded copy, whatever the rank), dev_batches()
    dev_size, both batch_size at a time.  train_hparams are the WHOLE job's, as RankTrainerDDP takes them.  Each call opens its file anew: train_batches(epoch) gives the same batches in the same order again,
    which resuming from a checkpoint relies on."""
    batch_size = int(train_hparams['batch_size'])
    if world <= 1:
        rank = None                      # one rank: write_shuffled_copies(world=1) wrote the un-sharded names
    train_size = int(train_hparams['train_size']) // (world if rank is not None else 1)
    dev_fname = os.path.join(data_path, _basenames(train_hparams)[1] + '.jsonl')

    def train_batches(epoch):
        return JsonlRankBatches(shuffled_fname(model_path, train_hparams, epoch, rank), train_size, batch_size, tokenizer, align_type)

    def dev_batches():
        return JsonlRankBatches(dev_fname, int(train_hparams['dev_size']), batch_size, tokenizer, align_type)

    return train_batches, dev_batches
