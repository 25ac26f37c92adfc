"""Special-token table the decode driver needs (ids only; the tokenizer stays on the caller's side).

The reference looks these up by name in ./tokenizer.json
(/root/reference/src/transcribe.rs:179-185, src/token.rs:26-30, :267-295) and builds
the special-token mask by calling `is_special` on every vocab id
(transcribe.rs:243-251).  No tokenizer.json exists here, so the ids of the standard
Whisper vocabularies are tabulated from the published vocab layout; a caller that
does own a tokenizer passes its own table.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np


LANGUAGES = ("en zh de es ru ko fr ja pt tr pl ca nl ar sv it id hi fi vi he uk el ms cs ro da hu ta no th ur hr bg lt la "
             "mi ml cy sk te fa lv bn sr az sl kn et mk br eu is hy ne mn bs kk sq sw gl mr pa si km sn yo so af oc ka be "
             "tg sd gu am yi lo uz fo ht ps tk nn mt sa lb my bo tl mg as tt ln ha ba jw su").split()   # token.rs:50-60


@dataclass
class SpecialTokens:
    start_of_transcript: int
    language: int
    transcribe: int
    no_timestamps: int
    end_of_text: int
    is_special: np.ndarray      # uint8 [V]: 1 where tokenizer.decode([id], skip_special=True) == ""
    start_of_prev: int = -1     # <|startofprev|> (transcribe.rs:181); only the optional prompt-conditioning mode uses it
    language_ids: tuple = ()    # every language token of the vocabulary, ascending (empty: English-only); detect_language
    no_speech: int = -1         # <|nospeech|> (<|nocaptions|> in the original vocabulary files); -1: none
    timestamp_begin: int = 0    # <|0.00|>: ids [timestamp_begin, timestamp_begin + n_timestamps) are the timestamp tokens
    n_timestamps: int = 0       # 1501 in Whisper's vocabularies (0.00 .. 30.00 s in 0.02 s steps); 0: the vocabulary has none

    @staticmethod
    def for_vocab(n_vocab: int, language_index: int = 0) -> "SpecialTokens":
        """Standard Whisper layouts: 51864 (.en) / 51865 (multilingual); any other size
        (synthetic test vocabularies) places the specials in the last 16 ids."""
        if n_vocab == 51864:        # gpt2 + <|endoftext|>=50256, sot=50257, 99 langs, translate ...
            eot, sot = 50256, 50257
            lang0, transcribe, notimestamps = 50258, 50358, 50362
            sop = 50360
            langs, nsp = (), 50361           # the .en vocabulary keeps the slots, the checkpoint knows one language
            ts0, nts = 50363, 1501
        elif n_vocab == 51865:
            eot, sot = 50257, 50258
            lang0, transcribe, notimestamps = 50259, 50359, 50363
            sop = 50361
            langs, nsp = tuple(range(50259, 50358)), 50362   # 99 slots between sot and <|translate|>
            ts0, nts = 50364, 1501
        else:
            assert n_vocab >= 32
            eot = n_vocab - 16
            sot, lang0, transcribe, notimestamps = eot + 1, eot + 2, eot + 4, eot + 6
            sop = eot + 5
            language_index = 0
            langs, nsp = (eot + 2, eot + 3), -1     # two language slots (en, zh), no no-speech token
            ts0, nts = 0, 0                         # ... and no timestamp block (a test names a range of its own)
        is_special = np.zeros(n_vocab, dtype=np.uint8)
        is_special[eot:] = 1
        return SpecialTokens(sot, lang0 + language_index, transcribe, notimestamps, eot, is_special, sop, langs, nsp, ts0, nts)


# Whisper's non-speech symbols (tokenizer.py: non_speech_tokens): suppressed so that the transcript carries no annotations
NON_SPEECH_SYMBOLS = tuple('"#()*+/:;<=>@[\\]^_`{|}~「」『』') + (
    "<<", ">>", "<<<", ">>>", "--", "---", "-(", "-[", "('", '("', "((", "))", "(((", ")))", "[[", "]]", "{{", "}}", "♪♪", "♪♪♪",
    "♩", "♪", "♫", "♬", "♭", "♮", "♯")


def default_suppress(st: SpecialTokens, tokenizer: "TokenizerAdapter" = None):
    """Whisper's default static masks for timestamp decoding, (suppress, suppress_first) as uint8 [V]: suppress = every
    special token but end-of-text and the timestamps -- with a tokenizer also the non-speech symbols (the ids that encode
    a symbol alone or behind a space) --; suppress_first = end-of-text -- with a tokenizer also the blank " "."""
    V = len(st.is_special)
    sup = (np.asarray(st.is_special) != 0).astype(np.uint8)
    sup[st.end_of_text] = 0
    sup[st.timestamp_begin:st.timestamp_begin + st.n_timestamps] = 0
    first = np.zeros(V, dtype=np.uint8)
    first[st.end_of_text] = 1
    if tokenizer is not None:
        for sym in NON_SPEECH_SYMBOLS:
            for text in (sym, " " + sym):
                ids = tokenizer.tok.encode(text, add_special_tokens=False).ids
                if len(ids) == 1 and 0 <= ids[0] < V:
                    sup[ids[0]] = 1
        ids = tokenizer.tok.encode(" ", add_special_tokens=False).ids
        if len(ids) == 1:
            first[ids[0]] = 1
    return sup, first


# ---- tokenizer integration (src/token.rs) -------------------------------------------------------------------

def special_token_name(kind: str, language: str = "en") -> str:
    """`SpecialToken::to_string` (token.rs:280-295)."""
    return {"endoftext": "<|endoftext|>", "startoftranscript": "<|startoftranscript|>", "translate": "<|translate|>",
            "transcribe": "<|transcribe|>", "startoflm": "<|startoflm|>", "startofprev": "<|startofprev|>",
            "nospeech": "<|nospeech|>", "notimestamps": "<|notimestamps|>", "language": f"<|{language}|>"}[kind]


class TokenizerAdapter:
    """The calls transcribe.rs makes on `Gpt2Tokenizer` (token.rs:12-48), over a HuggingFace `tokenizers.Tokenizer`
    (the crate the reference wraps, Cargo.lock:3504-3505) loaded from a `tokenizer.json`."""

    def __init__(self, tokenizer):
        self.tok = tokenizer

    @staticmethod
    def from_file(path: str = "tokenizer.json") -> "TokenizerAdapter":      # token.rs:13-19
        import tokenizers
        return TokenizerAdapter(tokenizers.Tokenizer.from_file(path))

    def special_token(self, name: str):                                     # token.rs:26-30
        return self.tok.token_to_id(name)

    def decode(self, tokens, skip_special: bool = True) -> str:             # token.rs:32-35
        return self.tok.decode([int(t) for t in tokens], skip_special_tokens=skip_special)

    def encode(self, text: str) -> list:
        """The ids of `text`, without added special tokens (Whisper's tokenizer.encode: what an initial prompt goes through)."""
        return [int(t) for t in self.tok.encode(text, add_special_tokens=False).ids]

    def is_special(self, token: int) -> bool:                               # token.rs:37-43
        try:
            return self.tok.decode([int(token)], skip_special_tokens=True) == ""
        except Exception:
            return False

    def vocab_size(self) -> int:                                            # token.rs:45-47
        return self.tok.get_vocab_size(with_added_tokens=True)

    def special_tokens(self, language: str = "en") -> SpecialTokens:
        """The five ids transcribe.rs:179-185 looks up and the mask transcribe.rs:243-251 builds by decoding every
        vocabulary id -- built ONCE here (the reference rebuilds it for every window)."""
        ids = {}
        for kind in ("startoftranscript", "language", "transcribe", "notimestamps", "endoftext"):
            v = self.special_token(special_token_name(kind, language))
            if v is None:
                raise KeyError(f"tokenizer has no {special_token_name(kind, language)}")
            ids[kind] = int(v)
        mask = np.array([1 if self.is_special(t) else 0 for t in range(self.vocab_size())], dtype=np.uint8)
        sop = self.special_token(special_token_name("startofprev"))
        return SpecialTokens(ids["startoftranscript"], ids["language"], ids["transcribe"], ids["notimestamps"],
                             ids["endoftext"], mask, -1 if sop is None else int(sop),
                             tuple(t for _, t in self.language_tokens()), self.no_speech_token(), *self.timestamp_range())

    def timestamp_range(self):
        """(id of <|0.00|>, number of consecutive <|x.xx|> tokens from it); (0, 0) when the tokenizer has none."""
        t0 = self.special_token("<|0.00|>")
        if t0 is None:
            return 0, 0
        n = 0
        while self.special_token("<|%.2f|>" % (0.02 * n)) == int(t0) + n:
            n += 1
        return int(t0), n

    def language_tokens(self):
        """(abbreviation, id) of every language token the tokenizer knows, in LANGUAGES order."""
        known = [(name, self.special_token(special_token_name("language", name))) for name in LANGUAGES]
        return [(name, int(t)) for name, t in known if t is not None]

    def no_speech_token(self) -> int:
        """<|nospeech|>, or its name in the original vocabulary files, <|nocaptions|>; -1: none."""
        for name in (special_token_name("nospeech"), "<|nocaptions|>"):
            t = self.special_token(name)
            if t is not None:
                return int(t)
        return -1
