"""The residual S2VT captioner under its own name.

``from s2vt_amd.residual import Video_Caption_Generator`` is the class residual_tf_s2vt.py:53-266 defines: tf_s2vt.py's model with
one more line at every decode step -- ``output2 = output1 + output2`` ahead of ``logit_words = tf.nn.xw_plus_b(output2,
embed_word_W, embed_word_b)`` in build_model (:149-151), build_generator (:206-208) and build_sampler (:263-265).  The encode steps,
the variables, their TF names and the checkpoint layout are tf_s2vt.py's, so a checkpoint trained with either script loads into
either class (what it then computes differs).  LSTM2's recurrent state stays the un-summed h'; only the operand of the vocabulary
projection changes.

Everything is model.Video_Caption_Generator built with ``residual=True``: build_model / build_generator / build_sampler /
build_multinomial_sampler / build_loss / minimize / reinforce_train_op, sample, beam_search, xe_update, reinforce_update, mixed_update
and e2e.EndToEnd.  mix_sample, scheduled_update, build_mix_sample and build_scheduled_model raise ValueError: the reference has no
residual form of those graphs and the library refuses the model bit there.
"""
from __future__ import annotations

from . import model as _model


class Video_Caption_Generator(_model.Video_Caption_Generator):
    def __init__(self, dim_image, n_words, word_dim, lstm_dim, batch_size, n_lstm_steps, n_video_lstm_step,
                 n_caption_lstm_step, bias_init_vector=None, loss_weight=1, decay_value=0.00005, dropout_rate=0.9, **kw):
        kw["residual"] = True
        super().__init__(dim_image, n_words, word_dim, lstm_dim, batch_size, n_lstm_steps, n_video_lstm_step,
                         n_caption_lstm_step, bias_init_vector=bias_init_vector, loss_weight=loss_weight, decay_value=decay_value,
                         dropout_rate=dropout_rate, **kw)
