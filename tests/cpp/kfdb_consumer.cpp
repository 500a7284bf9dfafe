// A plain C++ consumer of omv_adapt::KeyFrameDatabase (include/omv_adapters.hpp) with the call shape of
// LoopClosing::NewDetectCommonRegions (src/LoopClosing.cc:562: mpKeyFrameDB->DetectNBestCandidates(mpCurrentKF,
// vpLoopBowCand, vpMergeBowCand, 3)) and Tracking::Relocalization (src/Tracking.cc:3551: vpCandidateKFs =
// mpKeyFrameDB->DetectRelocalizationCandidates(&mCurrentFrame, mpAtlas->GetCurrentMap())).
// The map is made here: 40 keyframes along a trajectory, consecutive ones sharing most of their words, the last ten
// in a second map; the current keyframe revisits keyframe 7 and is connected to its own predecessors.  Prints one line
//   loop <n> first <id> merge <n> first <id> reloc <n> first <id> after_erase_first <id>
// and exits 0 when the planted revisit (and, in the other map, its twin) is found.
#include <cstdio>
#include <random>
#include <vector>

#include "omv_adapters.hpp"

struct KeyFrame {   // the caller's type; the adapter only uses its address
    int mnId = 0, map = 0;
    std::vector<int32_t> words;
    std::vector<double> values;
};

static const int kStride = 256;

static void normalise(KeyFrame &k) {
    double norm = 0.0;
    for (double v : k.values) norm += v;
    for (double &v : k.values) v /= norm;
}

int main() {
    try {
        std::mt19937 rng(11);
        std::uniform_real_distribution<double> W(0.5, 5.0);
        const int nKF = 40, nWords = 4000, perKF = 120;
        std::vector<KeyFrame> kfs(nKF + 1);
        std::vector<uint8_t> used(nWords, 0);
        std::vector<int32_t> cur;
        for (int i = 0; i < nKF; i++) {   // a sliding set of words: 80 % survive from one keyframe to the next
            std::vector<int32_t> next;
            for (int32_t w : cur)
                if (rng() % 100 < 80) next.push_back(w); else used[w] = 0;
            while ((int)next.size() < perKF) {
                const int32_t w = (int32_t)(rng() % nWords);
                if (!used[w]) used[w] = 1, next.push_back(w);
            }
            cur = next;
            std::sort(cur.begin(), cur.end());
            kfs[i].mnId = i + 1, kfs[i].map = i < 30 ? 0 : 1, kfs[i].words = cur;
            for (size_t k = 0; k < cur.size(); k++) kfs[i].values.push_back(W(rng));
            normalise(kfs[i]);
        }
        kfs[35].words = kfs[7].words, kfs[35].values = kfs[7].values;   // the same place seen in the other map
        KeyFrame &current = kfs[nKF];   // mpCurrentKF: keyframe 7's words, new weights, connected to 27..29
        current.mnId = nKF + 1, current.map = 0, current.words = kfs[7].words;
        for (size_t k = 0; k < current.words.size(); k++) current.values.push_back(kfs[7].values[k] * (0.9 + 0.2 * (rng() % 100) / 100.0));
        normalise(current);

        // BowVectors on the device in the layout omv_bow_transform leaves
        std::vector<int32_t> hw((size_t)(nKF + 1) * kStride, -1), hn(nKF + 1);
        std::vector<double> hv((size_t)(nKF + 1) * kStride, 0.0);
        for (int i = 0; i <= nKF; i++) {
            hn[i] = (int32_t)kfs[i].words.size();
            for (int k = 0; k < hn[i]; k++) hw[(size_t)i * kStride + k] = kfs[i].words[k], hv[(size_t)i * kStride + k] = kfs[i].values[k];
        }
        omv_adapt::DeviceArray<int32_t> dw, dn;
        omv_adapt::DeviceArray<double> dv;
        dw.upload(hw.data(), hw.size(), nullptr), dv.upload(hv.data(), hv.size(), nullptr), dn.upload(hn.data(), hn.size(), nullptr);
        omv_adapt::hip_check(hipStreamSynchronize(nullptr), "hipStreamSynchronize");

        omv_adapt::KeyFrameDatabase<KeyFrame> db(64, kStride, kStride);
        for (int i = 0; i < nKF; i++) db.add(&kfs[i], kfs[i].map, dw.p + (size_t)i * kStride, dv.p + (size_t)i * kStride, dn.p + i, kStride);
        std::vector<omv_adapt::KfdbKeyFrameState<KeyFrame>> state(nKF);
        for (int i = 0; i < nKF; i++) {   // covisibility: the neighbours along the trajectory, nearest first
            state[i].kf = &kfs[i];
            for (int d = 1; d <= 5; d++) {
                if (i - d >= 0) state[i].best_covisibles.push_back(&kfs[i - d]);
                if (i + d < nKF) state[i].best_covisibles.push_back(&kfs[i + d]);
            }
        }
        db.refresh(state);

        omv_adapt::KfdbQuery<KeyFrame> q;
        q.mnId = (long unsigned int)current.mnId, q.map_id = current.map;
        q.connected = {&kfs[27], &kfs[28], &kfs[29]};
        q.bow_word = dw.p + (size_t)nKF * kStride, q.bow_value = dv.p + (size_t)nKF * kStride, q.bow_n = dn.p + nKF, q.stride = kStride;
        std::vector<KeyFrame *> vpLoopBowCand, vpMergeBowCand;
        db.DetectNBestCandidates(q, vpLoopBowCand, vpMergeBowCand, 3);

        omv_adapt::KfdbQuery<KeyFrame> f = q;   // Tracking::Relocalization: the frame's id, the current map
        f.mnId = 1000, f.connected.clear();
        const std::vector<KeyFrame *> vpCandidateKFs = db.DetectRelocalizationCandidates(f);

        db.erase(&kfs[7]);   // SetBadFlag: out of the database, out of the candidates
        q.mnId++;
        std::vector<KeyFrame *> loop2, merge2;
        db.DetectNBestCandidates(q, loop2, merge2, 3);

        const int l0 = vpLoopBowCand.empty() ? -1 : vpLoopBowCand[0]->mnId, m0 = vpMergeBowCand.empty() ? -1 : vpMergeBowCand[0]->mnId;
        const int r0 = vpCandidateKFs.empty() ? -1 : vpCandidateKFs[0]->mnId, e0 = loop2.empty() ? -1 : loop2[0]->mnId;
        std::printf("loop %zu first %d merge %zu first %d reloc %zu first %d after_erase_first %d\n", vpLoopBowCand.size(), l0,
                    vpMergeBowCand.size(), m0, vpCandidateKFs.size(), r0, e0);
        bool ok = l0 == 8 && m0 == 36 && r0 == 8 && e0 != 8 && e0 != -1 && vpLoopBowCand.size() <= 3 && vpMergeBowCand.size() <= 3;
        for (KeyFrame *k : vpLoopBowCand) ok = ok && k->map == 0 && k->mnId < 28;
        for (KeyFrame *k : vpMergeBowCand) ok = ok && k->map == 1;
        for (KeyFrame *k : vpCandidateKFs) ok = ok && k->map == 0;
        return ok ? 0 : 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "kfdb_consumer: %s\n", e.what());
        return 2;
    }
}
