"""Extractor pipeline.  Mirrors offmark.video.extractor.Extractor
(reference src/offmark/video/extractor.py:11-34): ``Extractor(frame_reader, frame_extractor,
degenerator).start()`` logs each frame's recovered payload at INFO.

Extension: the payloads are also kept in ``self.patterns`` (the reference's
PatternCollectorExtractor, tests/segment_mark_detect_hls.py:119-161, re-implements the loop just to
collect them) and ``most_common()`` gives that class's (pattern, frequency) vote.

Batched GPU path when ``frame_extractor`` offers ``decode_frames_u8`` and the degenerator offers
``degenerate_counts`` (HIP DctDecoder + DeShuffler/DeGrayScale); generic per-frame path otherwise.

Build extension (not reference semantics): ``Extractor(..., soft=True)`` also brings every batch's soft sums back
(the decoder's ``decode_soft_frames_u8`` / ``decode_soft_planes_yuv420``, int64 [n, L]; a second read-out pass over each
batch, next to the hard one) and keeps them in ``self.soft_sums``; ``soft_payload()`` adds them over the frames seen and reads each position by the sign of its total
(dist.vote.soft_vote).  ``patterns``, ``most_common()`` and the log lines stay the reference's hard decision.
"""
import logging

import numpy as np

from ..common.__logging import trace
from ..dist.vote import soft_vote, vote
from .color import bgr2yuv

logger = logging.getLogger(__name__)


class Extractor:
    def __init__(self, frame_reader, frame_extractor, degenerator, batch_frames=64, soft=False):
        self.frame_reader = frame_reader
        self.frame_extractor = frame_extractor
        self.degenerator = degenerator
        self.batch_frames = batch_frames
        self.patterns = []
        self.soft = bool(soft)
        self.soft_sums = None          # soft=True: int64 [frames seen, L], in frame order

    @trace(logger)
    def start(self):
        batched = hasattr(self.frame_extractor, "decode_frames_u8") and hasattr(self.degenerator, "degenerate_counts")
        if self.soft and not (batched and hasattr(self.frame_extractor, "decode_soft_frames_u8")
                              and hasattr(self.frame_extractor, "decode_soft_planes_yuv420")):
            raise ValueError("soft=True needs the batched path and a decoder with decode_soft_frames_u8 / decode_soft_planes_yuv420")
        if batched:
            self.__run_batched()
        else:
            while True:
                in_frame = self.frame_reader.read()
                if in_frame is None:
                    logger.info("End of input stream")
                    break
                self.__check_frame(in_frame)
        self.frame_reader.close()
        logger.info("Done")

    def most_common(self):
        """(most common whole pattern, its frequency) over the frames seen, or (None, None)."""
        flat = [np.asarray(p).reshape(-1) for p in self.patterns]
        return vote(np.stack(flat)) if flat else (None, None)

    def soft_payload(self):
        """Build extension: the payload read from the soft sums of all frames seen (soft=True), uint8 [L]."""
        if self.soft_sums is None:
            raise ValueError("soft_payload() needs Extractor(..., soft=True) and a finished start()")
        return soft_vote(self.soft_sums, self.degenerator.payload_idx)[0]

    def __run_batched(self):
        """The same three-stream pipeline as the Embedder's (offmark.video.pipeline), two batches in flight: while
        batch k's frames upload and its kernels run, batch k-1's counts come back and are degenerated on the host.
        Only [n, L] int32 counts travel device -> host."""
        from . import pipeline as pl
        dec = self.frame_extractor
        eng = dec.engine
        L = self.degenerator.payload_len
        reader = self.frame_reader
        if not (hasattr(reader, "height") and hasattr(reader, "width")):
            reader = pl.PeekedReader(reader)
            if reader.first is None:
                logger.info("End of input stream")
                return
        H, W = int(reader.height), int(reader.width)
        fmt = pl.pix_fmt_of(reader)
        planar = fmt != "rgb24" and hasattr(dec, "decode_planes_yuv420")

        def process(dev_in, dev_out):
            if planar:
                counts, _ = dec.decode_planes_yuv420(dev_in.view(dev_in.shape[0], -1), H, W, L, layout=pl.PLANAR_LAYOUT[fmt])
            else:
                counts, _ = dec.decode_frames_u8(pl.to_rgb_on_device(eng, dev_in, fmt, H, W), L)
            dev_out.copy_(counts)

        outer = self
        # length of the decoder's bit vector: H*W//64 for the DCT codec and DwtDctSvd(blk=4), H*W//256 for DwtDctSvd(blk=8)
        n_bits = dec.bits_per_frame(H, W) if hasattr(dec, "bits_per_frame") else H * W // 64

        class Sink:
            def deliver(self, counts):
                for out in outer.degenerator.degenerate_counts(counts, n_bits):
                    outer.patterns.append(out)
                    logger.info(out)

        if self.soft:
            self.__run_soft(pl, reader, fmt, planar, H, W, L, process, Sink())
        else:
            pl.StagedPipeline(eng.device, reader, pl.batch_size(self.batch_frames, pl.frame_shape(fmt, H, W)), pl.frame_shape(fmt, H, W),
                              (L,), np.int32).run(process, Sink())
        logger.info("End of input stream")

    def __run_soft(self, pl, reader, fmt, planar, H, W, L, process, sink):
        """soft=True: the same pipeline with one int64 [n, 2, L] array back per batch -- [:, 0] the hard path's counts (``process``
        and ``sink`` are the hard path's own, unchanged), [:, 1] the soft sums of a second read-out pass over the batch."""
        dec = self.frame_extractor
        batches = []

        def process_both(dev_in, dev_out):
            process(dev_in, dev_out[:, 0])
            if planar:
                sums = dec.decode_soft_planes_yuv420(dev_in.view(dev_in.shape[0], -1), H, W, L, layout=pl.PLANAR_LAYOUT[fmt])
            else:                                          # rgb24: a soft decoder has the planar call, so planes never come this way
                sums = dec.decode_soft_frames_u8(dev_in, L)
            dev_out[:, 1].copy_(sums)

        class Both:
            def deliver(self, both):
                batches.append(both[:, 1].copy())          # the landing buffer is reused
                sink.deliver(both[:, 0].astype(np.int32))

        pl.StagedPipeline(dec.engine.device, reader, pl.batch_size(self.batch_frames, pl.frame_shape(fmt, H, W)), pl.frame_shape(fmt, H, W),
                          (2, L), np.int64).run(process_both, Both())
        self.soft_sums = np.concatenate(batches) if batches else np.zeros((0, L), np.int64)

    def __check_frame(self, frame_rgb):
        wm_frame_yuv = bgr2yuv(frame_rgb.astype(np.float32))
        frame_yuv = self.frame_extractor.decode(wm_frame_yuv)
        out = self.degenerator.degenerate(frame_yuv)
        self.patterns.append(out)
        logger.info(out)
