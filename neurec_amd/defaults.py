"""Default configuration values, and a writer that materialises them as the ini files the
reference ships (`NeuRec.properties`, `conf/<Model>.properties`) for a fresh working directory.
Existing files written for the reference are read unchanged; this module only supplies
defaults when there are none."""
import os

LIBRARY = [
    ("recommender", "MF"), ("config_dir", "./conf"), ("gpu_id", "0"), ("gpu_mem", "0.5"),
    ("data.input.path", "dataset"), ("data.input.dataset", "ml-100k"),
    ("data.column.format", "UIRT"), ("data.convert.separator", "'\\t'"),
    ("user_min", "0"), ("item_min", "0"), ("splitter", "ratio"), ("ratio", "0.8"),
    ("by_time", "False"), ("metric", '["Precision", "Recall", "NDCG", "MAP", "MRR"]'),
    ("topk", "[10, 20]"), ("group_view", "None"), ("rec.evaluate.neg", "0"),
    ("test_batch_size", "128"), ("num_thread", "8"),
]

MODELS = {
    "MF": [("epochs", "300"), ("batch_size", "512"), ("embedding_size", "64"), ("reg_mf", "0.0"),
           ("learning_rate", "0.001"), ("learner", "adam"), ("num_negatives", "1"),
           ("is_pairwise", "True"), ("loss_function", "bpr"), ("init_method", "normal"),
           ("stddev", "0.01"), ("verbose", "1")],
    "LightGCN": [("lr", "0.01"), ("reg", "1e-3"), ("embed_size", "64"), ("n_layers", "6"),
                 ("batch_size", "1024"), ("epochs", "500"), ("n_fold", "100"),
                 ("adj_type", "pre")],
    "NGCF": [("epochs", "500"), ("batch_size", "512"), ("embedding_size", "16"),
             ("layer_size", "[16,16]"), ("learning_rate", "0.001"), ("node_dropout_flag", "False"),
             ("adj_type", "norm"), ("alg_type", "ngcf"), ("loss_function", "BPR"),
             ("learner", "adam"), ("reg", "0.0"), ("node_dropout_ratio", "0.1"),
             ("mess_dropout_ratio", "0.1"), ("embed_init_method", "xavier_normal"),
             ("weight_init_method", "xavier_normal"), ("stddev", "0.01"), ("verbose", "1")],
    "MultiVAE": [("epochs", "500"), ("p_dim", "[16,32]"), ("batch_size", "512"), ("reg", "0.0"),
                 ("learning_rate", "0.001"), ("activation", "tanh"),
                 ("loss_function", "multinominal-likelihood"), ("learner", "adam"),
                 ("anneal_cap", "0.2"), ("total_anneal_steps", "2000"),
                 ("weight_init_method", "xavier_normal"), ("bias_init_method", "tnormal"),
                 ("stddev", "0.01"), ("verbose", "1")],
    "Fossil": [("epochs", "100"), ("batch_size", "256"), ("embedding_size", "16"), ("regs", "[0.00,0.00,0.0]"),
               ("alpha", "0.5"), ("learning_rate", "0.001"), ("learner", "adagrad"), ("is_pairwise", "True"),
               ("high_order", "3"), ("num_neg", "4"), ("loss_function", "bpr"), ("init_method", "uniform"),
               ("stddev", "0.01"), ("verbose", "1")],
    "HRM": [("epochs", "3"), ("batch_size", "256"), ("embedding_size", "16"), ("reg_mf", "0"), ("topK", "10"),
            ("learning_rate", "0.001"), ("learner", "adam"), ("pre_agg", "max"), ("session_agg", "max"),
            ("high_order", "2"), ("num_neg", "4"), ("loss_function", "cross_entropy"), ("init_method", "normal"),
            ("stddev", "0.01"), ("verbose", "1")],
    "NPE": [("epochs", "100"), ("batch_size", "256"), ("embedding_size", "64"), ("reg", "0.1"),
            ("learning_rate", "0.001"), ("learner", "adam"), ("high_order", "3"), ("num_neg", "4"),
            ("loss_function", "cross_entropy"), ("init_method", "tnormal"), ("stddev", "0.01"), ("verbose", "1")],
    "FPMCplus": [("epochs", "500"), ("batch_size", "128"), ("embedding_size", "16"), ("weight_size", "16"),
                 ("high_order", "3"), ("reg_mf", "0.00001"), ("reg_w", "0.001"), ("learning_rate", "0.001"),
                 ("learner", "adam"), ("is_pairwise", "True"), ("num_neg", "4"), ("loss_function", "BPR"),
                 ("embed_init_method", "tnormal"), ("weight_init_method", "he_normal"), ("stddev", "0.01"),
                 ("verbose", "1")],
    "TransRec": [("epochs", "500"), ("batch_size", "1024"), ("embedding_size", "50"), ("reg_mf", "0.0"),
                 ("learning_rate", "0.001"), ("learner", "adam"), ("is_pairwise", "True"), ("num_neg", "4"),
                 ("loss_function", "bpr"), ("init_method", "tnormal"), ("stddev", "0.01"), ("verbose", "1")],
    "GRU4Rec": [("lr", "0.0001"), ("reg", "0.0"), ("layers", "[100]"), ("batch_size", "256"), ("loss", "top1"),
                ("hidden_act", "tanh"), ("final_act", "linear"), ("epochs", "1000")],
    "GRU4RecPlus": [("lr", "0.01"), ("reg", "0.0"), ("bpr_reg", "1.0"), ("layers", "[100]"), ("batch_size", "256"),
                    ("loss", "bpr_max"), ("hidden_act", "tanh"), ("final_act", "linear"), ("n_sample", "2048"),
                    ("sample_alpha", "0.75"), ("epochs", "1000")],
    "SASRec": [("lr", "0.001"), ("l2_emb", "0.0"), ("hidden_units", "50"), ("dropout_rate", "0.5"), ("max_len", "50"),
               ("num_blocks", "2"), ("num_heads", "1"), ("batch_size", "128"), ("epochs", "1000")],
    "Caser": [("lr", "0.001"), ("l2_reg", "0.001"), ("factors_num", "50"), ("seq_L", "5"), ("seq_T", "3"), ("nv", "4"),
              ("nh", "16"), ("dropout", "0.5"), ("neg_samples", "3"), ("batch_size", "256"), ("epochs", "1000")],
    "SRGNN": [("lr", "0.001"), ("L2", "1e-5"), ("hidden_size", "64"), ("batch_size", "100"), ("epochs", "500"),
              ("lr_dc", "0.1"), ("lr_dc_step", "3"), ("step", "1"), ("nonhybrid", "False"), ("max_seq_len", "200")],
    "NeuMF": [("epochs", "100"), ("batch_size", "256"), ("embedding_size", "16"), ("layers", "[64,32,16]"),
              ("reg_mf", "0"), ("reg_mlp", "0"), ("is_pairwise", "False"), ("num_neg", "4"),
              ("loss_function", "cross_entropy"), ("learning_rate", "0.001"), ("learner", "adam"),
              ("init_method", "normal"), ("stddev", "0.01"), ("verbose", "1"), ("mf_pretrain", "pretrain/GMF"),
              ("mlp_pretrain", "pretrain/MLP")],
    "MLP": [("epochs", "100"), ("batch_size", "256"), ("layers", "[64,32,16]"), ("reg_mlp", "0.0"),
            ("learning_rate", "0.001"), ("learner", "adam"), ("is_pairwise", "True"), ("num_neg", "4"),
            ("loss_function", "bpr"), ("verbose", "1"), ("init_method", "normal"), ("stddev", "0.01")],
    "CDAE": [("lr", "0.001"), ("reg", "0.001"), ("hidden_dim", "64"), ("dropout", "0.5"), ("num_neg", "5"),
             ("epochs", "5000"), ("batch_size", "32"), ("hidden_act", "sigmoid"),
             ("loss_func", "sigmoid_cross_entropy")],
    "DeepICF": [("pretrain_file", "None"), ("verbose", "1"), ("learner", "adam"), ("batch_size", "256"),
                ("epochs", "300"), ("layers", "[64,32,16]"), ("weight_size", "16"), ("embedding_size", "16"),
                ("data_alpha", "0"), ("regs", "[0.000001,0.000001,0.00001]"), ("regw", "[10,10]"), ("alpha", "0"),
                ("beta", "0.5"), ("num_neg", "4"), ("learning_rate", "0.001"), ("activation", "Relu"),
                ("algorithm", "1"), ("batch_norm", "1"), ("embed_init_method", "tnormal"),
                ("weight_init_method", "he_normal"), ("bias_init_method", "he_normal"), ("stddev", "0.01")],
    "ConvNCF": [("epochs", "100"), ("batch_size", "512"), ("embedding_size", "64"), ("regs", "[0.01,0,0]"),
                ("net_channel", "[32,32,32,32,32,32]"), ("lr_embed", "0.05"), ("lr_net", "0.05"),
                ("num_negatives", "4"), ("loss_function", "BPR"), ("keep", "1.0"), ("embed_init_method", "tnormal"),
                ("weight_init_method", "xavier_normal"), ("stddev", "0.01"), ("verbose", "1")],
    "CFGAN": [("reg_G", "0.001"), ("reg_D", "0.0"), ("lr_G", "0.0001"), ("lr_D", "0.0001"), ("ZR_ratio", "0.7"),
              ("ZP_ratio", "0.7"), ("ZR_coefficient", "0.03"), ("hiddenLayer_G", "[400]"), ("hiddenLayer_D", "[125]"),
              ("batchSize_G", "32"), ("batchSize_D", "64"), ("step_G", "1"), ("step_D", "1"), ("mode", "userBased"),
              ("opt_G", "adam"), ("opt_D", "adam"), ("epochs", "100"), ("verbose", "1")],
    "IRGAN": [("lr", "0.001"), ("factors_num", "20"), ("batch_size", "32"), ("epochs", "10"), ("d_epoch", "1"),
              ("g_epoch", "1"), ("g_reg", "0.0"), ("d_reg", "0.1/16"), ("d_tau", "0.2"),
              ("pretrain_file", "dataset/ml100k_saved_model.pkl")],
    "SBPR": [("learning_rate", "0.001"), ("embedding_size", "16"), ("learner", "adam"), ("loss_function", "bpr"),
             ("num_epochs", "500"), ("reg_mf", "0.01"), ("batch_size", "512"), ("social_file", "dataset/Ciao_u5_s2.uu"),
             ("init_method", "normal"), ("stddev", "0.01"), ("verbose", "1")],
    "JCA": [("hidden_neuron", "50"), ("epochs", "200"), ("f_act", "tanh"), ("g_act", "tanh"), ("batch_size", "256"),
            ("reg", "0"), ("learning_rate", "0.001"), ("corruption_level", "0.2"), ("learner", "adam"),
            ("margin", "0.15"), ("num_neg", "1"), ("init_method", "tnormal"), ("stddev", "0.01"), ("verbose", "1")],
    "APR": [("epochs", "30"), ("batch_size", "512"), ("embedding_size", "64"), ("reg", "0"), ("reg_adv", "1"),
            ("learning_rate", "0.001"), ("learner", "adam"), ("adv_epoch", "0"), ("adv", "grad"), ("eps", "0.5"),
            ("adver", "1"), ("init_method", "tnormal"), ("stddev", "0.01"), ("verbose", "1")],
}


def write_default_configs(directory, overrides=None, model_overrides=None):
    """Create NeuRec.properties and conf/*.properties under `directory`; returns the path of
    NeuRec.properties.  `overrides` / `model_overrides[model]` replace individual values."""
    os.makedirs(os.path.join(directory, "conf"), exist_ok=True)
    lib = dict(LIBRARY)
    lib.update(overrides or {})
    lib["config_dir"] = os.path.join(directory, "conf")
    path = os.path.join(directory, "NeuRec.properties")
    with open(path, "w") as f:
        f.write("[default]\n")
        for k, _ in LIBRARY:
            f.write("%s=%s\n" % (k, lib[k]))
        for k in lib:
            if k not in dict(LIBRARY):
                f.write("%s=%s\n" % (k, lib[k]))
    for model, items in MODELS.items():
        vals = dict(items)
        vals.update((model_overrides or {}).get(model, {}))
        with open(os.path.join(directory, "conf", model + ".properties"), "w") as f:
            f.write("[hyperparameters]\n")
            for k in vals:
                f.write("%s=%s\n" % (k, vals[k]))
    return path
