"""Drop-in for the reference's models/LanguageModel.py: same import path and class name, implemented by rnn_speech_amd."""
from rnn_speech_amd.language_model import LanguageModel  # noqa: F401
