// TEST INFRASTRUCTURE ONLY -- the lane emulator of tests/emul (smj_emul.cpp, included unchanged) plus the contact-readout slot
// (SMJ_SLOT_CONTACTS): env-major records [B][cap][SMJ_CR_WORDS], cap >= the build's NCON.  Never linked into libsmj.so.
#include "../emul/smj_emul.cpp"

extern "C" {
int emul_bind_contacts(emul_ctx* c, void* p, int cap) {
  if (p && cap < NCON) return -1;
  c->s.contacts = (float*)p;
  c->s.con_cap = cap;
  return 0;
}
int emul_contact_words() { return SMJ_CR_WORDS; }
}
