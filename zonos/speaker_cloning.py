"""zonos/speaker_cloning.py of the reference, on the HIP engine (zonos_amd/speaker.py)."""
from zonos_amd.speaker import SpeakerEmbedding, SpeakerEmbeddingLDA, logFbankCal  # noqa: F401
