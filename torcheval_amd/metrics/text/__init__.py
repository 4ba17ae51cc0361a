"""Text class metrics (parity: metrics/text/*.py)."""

from torcheval_amd.metrics.text._sum_states import _SumStates
from torcheval_amd.metrics.text.bleu import BLEUScore
from torcheval_amd.metrics.text.perplexity import Perplexity
from torcheval_amd.metrics.text.token_error_rate import TokenErrorRate  # noqa: F401  (not a reference name: kept out of __all__)
from torcheval_amd.metrics.text.token_rouge_l import TokenROUGEL  # noqa: F401  (not a reference name: kept out of __all__)
from torcheval_amd.metrics.text.word_error_rate import WordErrorRate
from torcheval_amd.metrics.text.word_information_lost import WordInformationLost
from torcheval_amd.metrics.text.word_information_preserved import WordInformationPreserved

__all__ = [
    "BLEUScore",
    "Perplexity",
    "WordErrorRate",
    "WordInformationLost",
    "WordInformationPreserved",
]
__doc_name__ = "Text Metrics"
__doc_extras__ = ["TokenErrorRate"]  # documented, not a reference name
__doc_more__ = ["TokenROUGEL"]  # likewise; K29's export test pins the list above
